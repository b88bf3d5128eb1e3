# -*- coding: utf-8 -*-
"""`ssq_conceft`, `algos.conceft_gpu` and `conceft_stft` with the product's own kernel and host code under the CPU
emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_conceft.py, run as they are -- the kernel
against its NumPy statement on every shape (each tile width and register count), the links to the two-step path, batch
and repeat, the layouts, the entry's refusals, and the transform end to end. CPU-only."""
import pytest
import emu_backend
import conceft
import test_gpu_conceft as T

EMU_N = 200            # the signal length of the end-to-end cases here (2048 on the GPU)


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('shape', conceft.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_statement_leaves_out_no_column(shape):
    """For the seeded inputs no ``|Vq|`` lies within 1e-6 of `gamma`: every column is compared."""
    for dtype in T.DTYPES:
        assert not T.case(shape, dtype)[5].any()


@pytest.mark.parametrize('average', ['abs', 'complex'])
@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('shape', conceft.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_vs_statement(S, shape, dtype, flipud, average):
    T.test_kernel_vs_statement(S, shape, dtype, flipud, average)


@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
def test_unit_projections_are_the_two_step_path_per_plane(S, flipud):
    T.test_unit_projections_are_the_two_step_path_per_plane(S, flipud)


def test_one_plane_one_projection_complex_is_indexed_sum(S):
    T.test_one_plane_one_projection_complex_is_indexed_sum(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    T.test_batch_equals_single_calls_and_repeats(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_column_below_gamma_gives_zeros(S, dtype):
    T.test_column_below_gamma_gives_zeros(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_output_unwritten(S):
    T.test_abi_refusals_leave_output_unwritten(S)


@pytest.mark.parametrize('dtype, average', [('float32', 'abs'), ('float64', 'complex')])
def test_conceft_stft_vs_statement_on_its_own_planes(S, dtype, average):
    T.test_conceft_stft_vs_statement_on_its_own_planes(S, dtype, average, N=EMU_N)


def test_seed_and_explicit_projections_give_the_same_bits(S):
    T.test_seed_and_explicit_projections_give_the_same_bits(S, N=EMU_N)


def test_two_tones_land_on_their_rows(S):
    T.test_two_tones_land_on_their_rows(S, N=EMU_N)
