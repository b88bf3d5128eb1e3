# -*- coding: utf-8 -*-
"""Caller-supplied layouts (views, strides, the conj / neg bits, offset base pointers, other dtypes,
odd gradient layouts, `out=` arguments) through the product's own host code and kernels under the
CPU emulator (tests/emu/, tests/emu_backend.py): cases of tests/test_gpu_input_layouts.py, run as
they are, that cover every layout and every function family once -- forward transforms, the
two-step reassignment, the inverses, gradients, `out=` validation. What the host layer does with a
view or a lazy conjugate is the same code with or without a GPU; what gfx950 does with a base
pointer aligned to an element only is for the GPU module to tell (x86 takes any address). CPU-only."""
import pytest
import emu_backend
import test_gpu_input_layouts as T


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('case', [('float32', 128, 32, 1501, 'fused', False),
                                  ('float64', 128, 32, 1501, 'rocfft', False)],
                         ids=lambda c: '-'.join(str(v) for v in c))
def test_stft_and_ssq_stft_input_layouts(S, orc, case, monkeypatch):
    T.test_stft_and_ssq_stft_input_layouts(S, orc, case, monkeypatch)


def test_cwt_and_ssq_cwt_input_layouts(S, orc, monkeypatch):
    T.test_cwt_and_ssq_cwt_input_layouts(S, orc, ('float32', 'log-piecewise', 8, 601, None), monkeypatch)


def test_float16_and_int32_signals(S):
    T.test_float16_and_int32_signals(S)


def test_reassignment_input_layouts(S, orc):
    T.test_reassignment_input_layouts(S, orc, 'float32', False)


def test_out_arguments_are_validated(S):
    T.test_out_arguments_are_validated(S, 'float32')


def test_inverse_cwt_input_layouts(S):
    T.test_inverse_cwt_input_layouts(S, 'float32')


def test_inverse_stft_input_layouts(S):
    T.test_inverse_stft_input_layouts(S, 'float32')


def test_incoming_gradient_layouts_inverses(S):
    T.test_incoming_gradient_layouts_inverses(S, 'float32')


def test_adjoint_entry_points_gradient_layouts(S):
    T.test_adjoint_entry_points_gradient_layouts(S, 'float32')


def test_input_side_gradient_layouts(S):
    T.test_input_side_gradient_layouts(S, 'float32')
