# -*- coding: utf-8 -*-
"""`ssq_stft2` (`ssq_stft2_phase`, `algos.phase_stft2_gpu`, the three plan executions, the ordered
reassignment) with the product's own kernels and host code under the CPU emulator (tests/emu/,
tests/emu_backend.py): cases of tests/test_gpu_ssq_stft2.py, run as they are, at sizes the emulator
finishes in seconds -- the map against its NumPy statement, `Tx` against the reassignment of the
returned `w`, the first-order fallback, the thresholds, the ABI's error paths. CPU-only."""
import pytest
import emu_backend
import test_gpu_ssq_stft2 as T


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    T._PLANES.clear()
    with emu_backend.emulated() as mod:
        yield mod
    T._PLANES.clear()                           # planes made here are the emulator's, not a GPU's


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('shape, dtype', [((640, 256, 16), 'float32'), ((1000, 96, 4), 'float64'),
                                          ((1000, 96, 4, 3), 'float32')],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_map_vs_numpy_statement(S, shape, dtype):
    T.test_map_vs_numpy_statement(S, shape, dtype)


@pytest.mark.parametrize('dtype, flipud', [('float32', False), ('float64', True)])
def test_tx_is_ordered_reassignment_of_w(S, dtype, flipud):
    T.test_tx_is_ordered_reassignment_of_w(S, dtype, flipud, N=301, n_fft=64, hop=2, B=2)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_first_order_fallback(S, dtype):
    T.test_first_order_fallback(S, dtype)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_fallback_matches_phase_stft(S, dtype):
    T.test_fallback_matches_phase_stft(S, dtype)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_all_zero_signal(S, dtype):
    T.test_all_zero_signal(S, dtype)


def test_abi_errors_leave_output_unwritten(S):
    T.test_abi_errors_leave_output_unwritten(S)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_offset_pointers_take_the_element_path(S, dtype):
    T.test_offset_pointers_take_the_element_path(S, dtype)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', T.second_order.PARENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_parent_bits(S, shape, dtype):
    T.test_parent_bits(S, shape, dtype)
