# -*- coding: utf-8 -*-
"""The batched, differentiable inverses with the product's own kernels and host code under the CPU
emulator (tests/emu/, tests/emu_backend.py): a handful of the cases of
tests/test_gpu_inverse_batched.py, run as they are, at sizes the emulator finishes in seconds -- the
fused inverse STFT and its backward, the composed route, the column-sum and band adjoints, the
autograd functions. CPU-only."""
import pytest
import emu_backend
import test_gpu_inverse_batched as T
import test_gpu_inverse as TI


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host
    import test_gpu_autograd
    monkeypatch.setattr(test_gpu_autograd, 'DEV', 'cpu')
    monkeypatch.setattr(TI, 'DEV', 'cpu')


@pytest.mark.parametrize('dtype,n_fft,hop,N', T.BATCH_SHAPES)
def test_istft_batch_equals_single(S, dtype, n_fft, hop, N):
    T.test_istft_batch_equals_single(S, dtype, n_fft, hop, N, 3)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_issq_batch_equals_single(S, dtype):
    T.test_issq_batch_equals_single(S, dtype, 3)


def test_istft_route(S):
    T.test_istft_route(S)


@pytest.mark.parametrize('n_fft,wcase,N,combos', [
    (128, 'default-hop3', 677, [(True, 1, 2), (False, 0, 0)]),
    (256, 'hann-n/4', 1317, [(True, 2, 0), (False, 1, 2)]),
    (1024, 'hann0.78-n/8', 3001, [(True, 1, 2)]),
    (2048, 'hann-n/8', 5157, [(False, 2, 0)]),
])
def test_fused_istft_vs_statement(S, n_fft, wcase, N, combos):
    T.check_istft_vs_statement(S, n_fft, wcase, N=N, combos=combos)


def test_fused_istft_small_window_norm(S):
    T.test_fused_istft_small_window_norm(S, 512, N=1500)


@pytest.mark.parametrize('case', [
    ('float32', 128, None, None, 1, 400, True, 1, 2, 'fused'),
    ('float32', 512, 'hann', None, 64, 1700, False, 2, 0, 'fused'),
    ('float32', 1024, 'hann', 800, 128, 3001, True, 0, 2, 'fused'),
    ('float64', 100, 'hann', None, 12, 537, True, 1, 2, 'rocfft'),
    ('float32', 101, None, None, 3, 400, False, 2, 0, 'rocfft'),
], ids=lambda c: '-'.join(str(v) for v in c))
def test_istft_gradient(S, case):
    T.check_istft_gradient(S, *case)


@pytest.mark.parametrize('dtype,n_fft,hop,N,modulated,win_exp', [
    ('float32', 256, 3, 700, True, 1), ('float64', 100, 7, 501, True, 0)])
def test_istft_adjoint_abi_vs_closed_form(S, dtype, n_fft, hop, N, modulated, win_exp):
    T.test_istft_adjoint_abi_vs_closed_form(S, dtype, n_fft, hop, N, modulated, win_exp)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_exact_adjoints(S, dtype):
    T.test_colsum_adjoint_is_exact(S, dtype, 300)
    T.test_colsum_adjoint_is_exact(S, dtype, 301)
    T.test_band_adjoint_is_exact(S, dtype, False)
    T.test_band_adjoint_is_exact(S, dtype, True)


def test_end_to_end(S):
    T.check_masked_stft_round_trip(S, 256, 64, 1317, 2)
    T.test_torch_stft_window_statement_matches_the_autograd_tests(S)
    T.check_icwt_cwt_dot_product(S, 'float32', 'log-piecewise', True, 2, N=300)
    T.check_icwt_cwt_dot_product(S, 'float64', 'linear', False, 0, N=300)
    T.check_issq_chain(S, 'ssq_cwt', 'float32', 2)
    T.check_issq_chain(S, 'ssq_stft', 'float64', 0)


def test_nothing_asked_nothing_changed(S):
    T.test_nothing_asked_nothing_changed(S)


@pytest.mark.parametrize('route', TI.CACHED_ROUTES)
def test_plan_cache_eviction_keeps_the_bits(S, route):
    TI.check_cache_eviction(S, route)
