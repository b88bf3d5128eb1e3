# -*- coding: utf-8 -*-
"""The backward passes of `stft`, `ssq_stft` and `ssq_cwt` with the product's own adjoint kernels and
host code under the CPU emulator (tests/emu/, tests/emu_backend.py): a few cases of
tests/test_gpu_autograd.py, run as they are, at sizes the emulator finishes in seconds -- the
fused LDS-transform adjoint, the composed route, the reassignment's gather, the autograd
functions. CPU-only."""
import pytest
import emu_backend
import test_gpu_autograd as T


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('case', [
    ('float32', 128, 3, 'wrap', True, None, 77, 1, True, 1., 'fused'),
    ('float32', 1024, 256, 'reflect', True, 800, 3001, 2, True, 1., 'fused'),
    ('float32', 1024, 1, 'wrap', True, None, 300, 0, False, 1., 'fused'),
    ('float32', 598, 7, 'reflect', True, None, 1000, 2, True, 1., 'fused-mixed-radix'),
    ('float64', 101, 4, 'symmetric', True, None, 150, 2, False, 3., 'rocfft'),
], ids=lambda c: '-'.join(str(v) for v in c[:8]))
def test_stft_gradient_vs_torch(S, case):
    T.test_stft_gradient_vs_torch(S, case)


@pytest.mark.parametrize('dtype,n_fft,hop,padtype,modulated,N', [
    ('float32', 256, 64, 'wrap', False, 1000),
    ('float32', 2048, 512, 'replicate', True, 3000),
    ('float64', 100, 3, 'reflect', True, 301),
])
def test_stft_adjoint_abi_vs_closed_form(S, dtype, n_fft, hop, padtype, modulated, N):
    T.test_stft_adjoint_abi_vs_closed_form(S, dtype, n_fft, hop, padtype, modulated, N)


@pytest.mark.parametrize('dtype,form', [('float32', 'cwt'), ('float64', 'stft')])
def test_ssqueeze_adjoint_is_the_gather(S, dtype, form):
    T.test_ssqueeze_adjoint_is_the_gather(S, dtype, form)


def test_ssq_gradients(S):
    T.test_ssq_stft_gradient(S, 'float32', 128, 2, 2)
    T.test_ssq_cwt_gradient(S, 'float32', 'log-piecewise', 0)
    T.test_ssq_gradient_vs_finite_difference(S, 'ssq_cwt')


def test_no_gradient_when_none_is_asked_for(S):
    T.test_no_gradient_when_none_is_asked_for(S)
