# -*- coding: utf-8 -*-
"""The backward of the CWT plan (`ssq_cwt_adjoint`, `CwtPlan.adjoint`, the gradient through `dWx`)
with the product's own kernels and host code under the CPU emulator (tests/emu/,
tests/emu_backend.py): a few cases of tests/test_gpu_autograd_cwt.py, run as they are, at sizes
the emulator finishes in seconds -- the staging, multiply-accumulate and unpadding kernels, the
chunk loop, the ABI's error paths, the autograd functions. CPU-only."""
import pytest
import emu_backend
import test_gpu_autograd_cwt as T


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
    ('float32', 'reflect', True, 300, 1., 3, False),
    ('float64', 'symmetric', False, 300, 1., 3, False),
    ('float32', 'replicate', False, 300, 4., 0, False),
    ('float32', None, True, 301, 2., 0, False),
    ('float64', 'zero', True, 301, .5, 0, True),
], ids=lambda c: '-'.join(str(v) for v in c))
def test_cwt_adjoint_vs_closed_form(S, case):
    T.test_cwt_adjoint_vs_closed_form(S, case)


def test_cwt_adjoint_argument_errors(S):
    T.test_cwt_adjoint_argument_errors(S)


@pytest.mark.parametrize('case', [
    ('float32', 'reflect', True, 300, 1., 2, False),
    ('float64', 'zero', False, 300, 2., 0, False),
], ids=lambda c: '-'.join(str(v) for v in c))
def test_cwt_gradient_through_dWx(S, case):
    T.test_cwt_gradient_through_dWx(S, case)


def test_cwt_adjoint_batch_and_repeat(S):
    T.test_cwt_adjoint_batch_and_repeat(S, 'float32', 'reflect', 300)


@pytest.mark.parametrize('which', ['cwt', 'ssq_cwt'])
def test_backward_builds_no_dense_bank(S, which):
    T.test_backward_builds_no_dense_bank(S, which)


def test_cwt_adjoint_abi(S):
    T.test_cwt_adjoint_abi(S)
