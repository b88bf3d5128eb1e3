# -*- coding: utf-8 -*-
"""`ssq_multi_squeeze_cwt`, `algos.multi_squeeze_cwt_gpu` and `msst_cwt` with the product's own kernel and host code
under the CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_msst_cwt.py, run as they are --
the kernel against its NumPy statement on every kind of table, both sides of every tile width and the most rows, the
column counts around the tiles, the row counts off the lanes, the crafted columns, the link to the linear kernel and to
`indexed_sum_onfly`, order, batch and repeat, the layouts, the refusals, the column sums, the transform end to end on a
shorter signal, and what it buys on the issue's signals. CPU-only."""
import pytest
import emu_backend
import test_gpu_msst_cwt as T

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
@pytest.mark.parametrize('case', T.TABLE_CASES, ids=lambda c: '%s_%d' % c[:2])
def test_tables(S, case, dtype):
    T.test_tables(S, case, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_tile_edges_and_most_rows(S, dtype):
    T.test_tile_edges_and_most_rows(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('cols', [16, 8, 4])
def test_column_counts_around_the_tiles(S, cols, dtype):
    T.test_column_counts_around_the_tiles(S, cols, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('rows', T.SMALL_ROWS)
def test_row_counts_off_the_lanes(S, rows, dtype):
    T.test_row_counts_off_the_lanes(S, rows, dtype)


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_crafted_columns(S, dtype, interp):
    T.test_crafted_columns(S, dtype, interp)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_half_positions_and_missing_neighbours(S, dtype):
    T.test_half_positions_and_missing_neighbours(S, dtype)


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_link_to_the_linear_kernel(S, dtype, interp):
    T.test_link_to_the_linear_kernel(S, dtype, interp)


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
def test_plane_layouts_and_python_refusals(S, dtype):
    T.test_plane_layouts_and_python_refusals(S, dtype)


def test_abi_refusals_leave_outputs_unwritten(S):
    T.test_abi_refusals_leave_outputs_unwritten(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_column_sums_are_kept(S, dtype):
    T.test_column_sums_are_kept(S, dtype)


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_msst_cwt_is_its_parts(S, dtype, order):
    T.test_msst_cwt_is_its_parts(S, dtype, order, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_inverse(S, dtype):
    T.test_inverse(S, dtype, N=EMU_N)


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('name', list(T.M.SIGNALS))
def test_sharpening(S, name, dtype):
    T.test_sharpening(S, name, dtype)                       # (the issue's signals: their own lengths here too)
