# -*- coding: utf-8 -*-
"""`ssq_conceft_cwt`, `algos.conceft_cwt_gpu` and `conceft_cwt` with the product's own kernel and host code under the
CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_conceft_cwt.py, run as they are -- the
kernel against its NumPy statement on every shape (each tile width and register count) and grid, the link to the
two-step path, the rows' weights, batch and repeat, the layouts, the entry's refusals, and the transform end to end.
Here too, on the CPU, the condition on the statement itself: it leaves out at most 1 % of the columns of any case.
CPU-only."""
import pytest
import emu_backend
import conceft_cwt as cc
import test_gpu_conceft_cwt as T

EMU_N = 256            # the signal length of the end-to-end cases here (2048 on the GPU)


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('grid', cc.GRIDS)
@pytest.mark.parametrize('shape', cc.SHAPES, ids=T.shape_id)
def test_statement_leaves_out_at_most_one_percent(shape, grid):
    """The columns with a point near `gamma` or near a bin's rounding boundary: at most 1 % of any case. A point is
    near a boundary with probability 2e-9 and near `gamma` with about 2e-6 times the density of ``|Wq|`` there, so for
    random planes a share of about 1e-4 is expected; with the seeds of `conceft_cwt.SEEDS` it is none. The count is
    recorded."""
    from conftest import report_measured
    for dtype in T.DTYPES:
        near = T.projections(shape, dtype, grid)[2]
        report_measured('conceft_cwt_excluded_%s_%s_%s' % (T.shape_id(shape), grid, dtype),
                        excluded_columns=int(near.sum()), columns=int(near.size))
        assert near.mean() <= .01


@pytest.mark.parametrize('average', ['abs', 'complex'])
@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('grid', cc.GRIDS)
@pytest.mark.parametrize('shape', cc.SHAPES, ids=T.shape_id)
def test_kernel_vs_statement(S, shape, grid, dtype, flipud, average):
    T.test_kernel_vs_statement(S, shape, grid, dtype, flipud, average)


@pytest.mark.parametrize('grid', cc.GRIDS)
def test_a_rows_weight_shows_where_its_terms_land(S, grid):
    T.test_a_rows_weight_shows_where_its_terms_land(S, grid)


@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
@pytest.mark.parametrize('grid', cc.GRIDS)
def test_one_plane_one_projection_complex_is_the_two_step_path(S, grid, flipud):
    T.test_one_plane_one_projection_complex_is_the_two_step_path(S, grid, flipud)


def test_zero_derivative_lands_in_bin_0(S):
    T.test_zero_derivative_lands_in_bin_0(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls_repeats_and_out(S, dtype):
    T.test_batch_equals_single_calls_repeats_and_out(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_output_unwritten(S):
    T.test_abi_refusals_leave_output_unwritten(S)


def test_ssq_conceft_is_unchanged(S):
    T.test_ssq_conceft_is_unchanged(S)


@pytest.mark.parametrize('dtype, B, scales', [('float32', 1, 'log-piecewise'), ('float64', 2, 'log'),
                                              ('float32', 2, 'log'), ('float64', 1, 'log-piecewise')])
def test_conceft_cwt_vs_statement_on_its_own_planes(S, dtype, B, scales):
    T.test_conceft_cwt_vs_statement_on_its_own_planes(S, dtype, B, scales, N=EMU_N)


def test_arguments(S):
    T.test_arguments(S, N=EMU_N)
