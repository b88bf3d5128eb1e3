# -*- coding: utf-8 -*-
"""`ssq_reassign_cwt`, `algos.reassign_cwt_gpu` and `reassign_cwt` with the product's own kernels and host code under the
CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_reassign_cwt.py, run as they are -- the
kernels against their NumPy statement on every shape, grid and `flipud`, the modes, order independence, the crafted
planes, conservation and the links to the siblings, the layouts, the entry's refusals, and the transform end to end.
CPU-only."""
import pytest
import emu_backend
import test_gpu_reassign_cwt as T

EMU_N = 512            # the signal length of the is-its-parts and impulse cases here (1024 on the GPU)


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
@pytest.mark.parametrize('flipud', [False, True], ids=['', 'flipud'])
@pytest.mark.parametrize('kind', T.GRIDS)
@pytest.mark.parametrize('idx', range(len(T.SHAPE_IDS)), ids=T.SHAPE_IDS)
def test_kernel_vs_statement(S, idx, kind, flipud, dtype):
    T.test_kernel_vs_statement(S, idx, kind, flipud, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('freq,time', [(True, False), (False, True), (False, False)], ids=['freq', 'time', 'neither'])
def test_modes(S, freq, time, dtype):
    T.test_modes(S, freq, time, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('idx', [T.TILE_PLUS_1, T.SCATTERED], ids=['tile_plus_1', 'scattered'])
def test_window_home_and_repeat_give_the_same_bits(S, idx, dtype):
    T.test_window_home_and_repeat_give_the_same_bits(S, idx, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_reversed_columns_give_the_same_bits(S, dtype):
    T.test_reversed_columns_give_the_same_bits(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls_and_conservation(S, dtype):
    T.test_batch_equals_single_calls_and_conservation(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('kind', T.GRIDS)
def test_rows_sent_to_given_bins_and_shifts(S, kind, dtype):
    T.test_rows_sent_to_given_bins_and_shifts(S, kind, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('kind', T.GRIDS)
def test_frequencies_off_the_grid_land_in_the_end_bins(S, kind, dtype):
    T.test_frequencies_off_the_grid_land_in_the_end_bins(S, kind, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_the_displacement_bound_is_per_row(S, dtype):
    T.test_the_displacement_bound_is_per_row(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_every_point_into_one_cell_pins_the_headroom(S, dtype):
    T.test_every_point_into_one_cell_pins_the_headroom(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_a_cell_that_a_float32_running_sum_would_lose(S, dtype):
    T.test_a_cell_that_a_float32_running_sum_would_lose(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_points_below_gamma_and_non_finite_points(S, dtype):
    T.test_points_below_gamma_and_non_finite_points(S, dtype)


def test_freq_mode_is_indexed_sum_of_the_energy(S):
    T.test_freq_mode_is_indexed_sum_of_the_energy(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_time_mode_is_the_stft_form_row_by_row(S, dtype):
    T.test_time_mode_is_the_stft_form_row_by_row(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_output_unwritten(S):
    T.test_abi_refusals_leave_output_unwritten(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_reassign_cwt_is_its_parts(S, dtype):
    T.test_reassign_cwt_is_its_parts(S, dtype, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_unit_impulse(S, dtype):
    T.test_unit_impulse(S, dtype, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_fm_tone_shares_are_ordered(S, dtype):
    T.test_fm_tone_shares_are_ordered(S, dtype)
