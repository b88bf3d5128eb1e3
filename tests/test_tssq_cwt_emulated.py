# -*- coding: utf-8 -*-
"""`ssq_time_reassign_cwt`, `algos.time_reassign_cwt_gpu` and `tssq_cwt` with the product's own kernels and host code
under the CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_tssq_cwt.py, run as they are -- the
kernels against their NumPy statement on every shape, order and schedule, the crafted planes, conservation and the link to
`reassign_cwt_gpu`, the layouts, the entry's refusals, and the transform end to end. CPU-only."""
import pytest
import emu_backend
import test_gpu_tssq_cwt as T

EMU_N = 512            # the signal length of the end-to-end cases here (1024 on the GPU)


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('idx', range(len(T.SHAPE_IDS)), ids=T.SHAPE_IDS)
def test_kernel_vs_statement(S, idx, dtype):
    T.test_kernel_vs_statement(S, idx, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('idx', [T.TILE_PLUS_1, T.MIXED], ids=['tile_plus_1', 'mixed_bounds'])
def test_window_and_repeat_give_the_same_bits(S, idx, dtype):
    T.test_window_and_repeat_give_the_same_bits(S, idx, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_reversed_columns_give_the_reversed_acc(S, dtype):
    T.test_reversed_columns_give_the_reversed_acc(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls_and_conservation(S, dtype):
    T.test_batch_equals_single_calls_and_conservation(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_rows_sent_to_given_shifts(S, dtype):
    T.test_rows_sent_to_given_shifts(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_the_displacement_bound_is_per_row(S, dtype):
    T.test_the_displacement_bound_is_per_row(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_the_window_edge_is_at_the_halo(S, dtype):
    T.test_the_window_edge_is_at_the_halo(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_every_point_of_a_row_into_one_cell_pins_the_headroom(S, dtype):
    T.test_every_point_of_a_row_into_one_cell_pins_the_headroom(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_cancelling_pairs_leave_the_small_terms_exact(S, dtype):
    T.test_cancelling_pairs_leave_the_small_terms_exact(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_rotation_alone_and_no_rotation(S, dtype):
    T.test_rotation_alone_and_no_rotation(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_points_below_gamma_and_non_finite_points(S, dtype):
    T.test_points_below_gamma_and_non_finite_points(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_unit_magnitudes_count_terms_like_reassign_cwt(S, dtype):
    T.test_unit_magnitudes_count_terms_like_reassign_cwt(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_output_unwritten(S):
    T.test_abi_refusals_leave_output_unwritten(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_tssq_cwt_is_its_parts(S, dtype):
    T.test_tssq_cwt_is_its_parts(S, dtype, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('kind', ['impulse', 'dispersive'])
def test_sharpening_against_the_restatement(S, kind, dtype):
    T.test_sharpening_against_the_restatement(S, kind, dtype, N=EMU_N)
