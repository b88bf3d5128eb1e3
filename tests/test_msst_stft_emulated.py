# -*- coding: utf-8 -*-
"""`ssq_multi_squeeze`, `algos.multi_squeeze_gpu` and `msst_stft` with the product's own kernel and host code under the
CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_msst_stft.py, run as they are -- the kernel
against its NumPy statement (fewer column counts per row count), the tile-width edges, the crafted columns, the link to
`indexed_sum_onfly`, order, batch and repeat, the layouts, the entry's refusals, the column sums, the transform end to
end on a shorter signal, and what it buys on the full-length signals. CPU-only."""
import pytest
import emu_backend
import test_gpu_msst_stft as T

EMU_N = 512            # the signal length of the end-to-end cases here (1024 on the GPU)
EMU_COLS = [1, 4, 5, 17, 70]


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
@pytest.mark.parametrize('rows', T.ROWS)
def test_kernel_vs_statement(S, rows, dtype):
    T.test_kernel_vs_statement(S, rows, dtype, cols=EMU_COLS)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('edge', T.TILE_EDGES)
def test_tile_width_edges(S, edge, dtype):
    T.test_tile_width_edges(S, edge, dtype)


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_crafted_columns(S, dtype, interp):
    T.test_crafted_columns(S, dtype, interp)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_half_positions_and_missing_neighbours(S, dtype):
    T.test_half_positions_and_missing_neighbours(S, dtype)


@pytest.mark.parametrize('flipud', [False, True])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_one_pass_is_indexed_sum(S, dtype, flipud):
    T.test_one_pass_is_indexed_sum(S, dtype, flipud)


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('name', ['one_bin', 'two_bins'])
def test_order(S, name, dtype, interp):
    T.test_order(S, name, dtype, interp)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    T.test_batch_equals_single_calls_and_repeats(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_outputs_unwritten(S):
    T.test_abi_refusals_leave_outputs_unwritten(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_column_sums_are_kept(S, dtype):
    T.test_column_sums_are_kept(S, dtype)


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_msst_stft_is_its_parts(S, dtype, order):
    T.test_msst_stft_is_its_parts(S, dtype, order, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_inverse(S, dtype):
    T.test_inverse(S, dtype, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_linear_chirp_is_sharpened(S, dtype):
    T.test_linear_chirp_is_sharpened(S, dtype)             # (the issue's signal: 1024 samples here too)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_fm_tone_is_sharpened(S, dtype):
    T.test_fm_tone_is_sharpened(S, dtype)
