# -*- coding: utf-8 -*-
"""`ssq_reassign2d`, `algos.reassign2d_gpu` and `reassign_stft` with the product's own kernels and host code under the
CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_reassign_stft.py, run as they are -- the
kernels against their NumPy statement on every shape, the crafted planes, order independence, conservation and the
links to the one-axis transforms, the layouts, the entry's refusals, and the transform end to end. CPU-only."""
import pytest
import emu_backend
import test_gpu_reassign_stft as T

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
@pytest.mark.parametrize('idx', range(len(T.SHAPE_IDS)), ids=T.SHAPE_IDS)
def test_kernel_vs_statement(S, idx, dtype):
    T.test_kernel_vs_statement(S, idx, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('idx', [4, 11], ids=['tile_plus_1', 'scattered'])
def test_no_window_and_repeat_give_the_same_bits(S, idx, dtype):
    T.test_no_window_and_repeat_give_the_same_bits(S, idx, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_permuted_columns_give_the_same_bits(S, dtype):
    T.test_permuted_columns_give_the_same_bits(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls(S, dtype):
    T.test_batch_equals_single_calls(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_identity_and_uniform_shift(S, dtype):
    T.test_identity_and_uniform_shift(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_reflection_and_drops(S, dtype):
    T.test_reflection_and_drops(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_every_point_into_one_cell_pins_the_headroom(S, dtype):
    T.test_every_point_into_one_cell_pins_the_headroom(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_points_below_gamma_and_non_finite_points(S, dtype):
    T.test_points_below_gamma_and_non_finite_points(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_order_independence_where_a_float_sum_fails(S, dtype):
    T.test_order_independence_where_a_float_sum_fails(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_conservation_and_links(S, dtype):
    T.test_conservation_and_links(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_time_mode_has_the_geometry_of_time_reassign_on_the_energy(S, dtype):
    T.test_time_mode_has_the_geometry_of_time_reassign_on_the_energy(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_output_unwritten(S):
    T.test_abi_refusals_leave_output_unwritten(S)


@pytest.mark.parametrize('hop', [1, 4])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_reassign_stft_is_its_parts(S, dtype, hop):
    T.test_reassign_stft_is_its_parts(S, dtype, hop, N=EMU_N)


@pytest.mark.parametrize('hop', [1, 8])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_fm_tone_shares_are_ordered(S, dtype, hop):
    T.test_fm_tone_shares_are_ordered(S, dtype, hop)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_impulse_column_share(S, dtype):
    T.test_impulse_column_share(S, dtype, N=EMU_N)
