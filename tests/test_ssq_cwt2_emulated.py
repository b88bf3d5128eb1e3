# -*- coding: utf-8 -*-
"""`ssq_cwt2` (`ssq_cwt2_phase`, `algos.phase_cwt2_gpu`, the three plan executions, the ordered
reassignment) with the product's own kernels and host code under the CPU emulator (tests/emu/,
tests/emu_backend.py): cases of tests/test_gpu_ssq_cwt2.py, run as they are, at sizes the emulator
finishes in seconds -- the map against its NumPy statement, `chirp_tol=inf` against `phase_cwt`, `Tx`
against the reassignment of the returned `w`, the all-zero signal, the ABI's error paths. CPU-only."""
import pytest
import emu_backend
import test_gpu_ssq_cwt2 as T


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


@pytest.mark.parametrize('shape, dtype', [((250, 20), 'float32'), ((250, 20), 'float64'), ((777, 37), 'float32'),
                                          ((250, 20, 3), 'float32')],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_map_vs_numpy_statement(S, shape, dtype):
    T.test_map_vs_numpy_statement(S, shape, dtype)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', [(3, 5, 7), (1, 33, 129)], ids=lambda s: 'x'.join(map(str, s)))
def test_map_on_random_planes_takes_all_three_branches(S, shape, dtype):
    T.test_map_on_random_planes_takes_all_three_branches(S, shape, dtype)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_infinite_chirp_tol_is_phase_cwt(S, dtype):
    T.test_infinite_chirp_tol_is_phase_cwt(S, dtype)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_impulse_falls_back(S, dtype):
    T.test_impulse_falls_back(S, dtype, N=256)


@pytest.mark.parametrize('dtype, flipud, ssq_freqs', [('float32', False, None), ('float64', True, 'linear'),
                                                      ('float32', True, 'linear')])
def test_tx_is_ordered_reassignment_of_w(S, dtype, flipud, ssq_freqs):
    T.test_tx_is_ordered_reassignment_of_w(S, dtype, flipud, ssq_freqs, N=201, nv=4, B=2)


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
