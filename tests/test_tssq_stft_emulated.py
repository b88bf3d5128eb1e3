# -*- coding: utf-8 -*-
"""`ssq_time_reassign`, `algos.time_reassign_gpu` and `tssq_stft` with the product's own kernel and host code under the
CPU emulator (tests/emu/, tests/emu_backend.py): the cases of tests/test_gpu_tssq_stft.py, run as they are -- the kernel
against its NumPy statement on every shape (the segment-sized ones with two rows), order and conflicts, batch and repeat,
the layouts, the entry's refusals, and the transform end to end on a shorter signal. CPU-only."""
import numpy as np
import pytest
import emu_backend
import tssq
import test_gpu_tssq_stft as T

EMU_N = 512            # the signal length of the end-to-end cases here (1024 on the GPU)
S_ROWS = 2             # rows of the segment-sized shapes here (3 on the GPU)


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.fixture(autouse=True)
def host_tensors(monkeypatch):
    monkeypatch.setattr(T, 'DEV', 'cpu')        # emulated "device" tensors live on the host


@pytest.mark.parametrize('s_rows', [S_ROWS, 3])
@pytest.mark.parametrize('idx', range(len(T.SHAPE_IDS)), ids=T.SHAPE_IDS)
def test_statement_leaves_out_no_point(S, idx, s_rows):
    """For the seeded inputs no ``|Sx|`` lies within 1e-6 of `gamma`: every row is compared, here and on the GPU."""
    for dtype in T.DTYPES:
        assert not T.case(T.shape_of(idx, s_rows), dtype)[3].any()
    for dtype in T.DTYPES:
        assert not T.case(T.BATCH_SHAPE, dtype)[3].any()


@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('idx', range(len(T.SHAPE_IDS)), ids=T.SHAPE_IDS)
def test_kernel_vs_statement(S, idx, dtype):
    T.test_kernel_vs_statement(S, idx, dtype, s_rows=S_ROWS)


@pytest.mark.parametrize('rot', ['none', 'own'])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_rotation_tables(S, dtype, rot):
    T.test_rotation_tables(S, dtype, rot)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_rotation_index_beyond_32_bits(S, dtype):
    T.test_rotation_index_beyond_32_bits(S, dtype)


@pytest.mark.parametrize('rot', ['none', 'default'])
@pytest.mark.parametrize('dtype', T.DTYPES)
@pytest.mark.parametrize('name', T.CONFLICTS)
def test_order_and_conflicts(S, name, dtype, rot):
    T.test_order_and_conflicts(S, name, dtype, rot)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    T.test_batch_equals_single_calls_and_repeats(S, dtype)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_plane_layouts(S, dtype):
    T.test_plane_layouts(S, dtype)


def test_abi_refusals_leave_output_unwritten(S):
    T.test_abi_refusals_leave_output_unwritten(S)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_row_sums_are_the_kept_coefficients(S, dtype):
    T.test_row_sums_are_the_kept_coefficients(S, dtype)


@pytest.mark.parametrize('hop', [1, 4])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_tssq_stft_is_its_parts(S, dtype, hop):
    T.test_tssq_stft_is_its_parts(S, dtype, hop, N=EMU_N)


@pytest.mark.parametrize('hop', [1, 4])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_impulse_is_reassigned_to_its_column(S, dtype, hop):
    T.test_impulse_is_reassigned_to_its_column(S, dtype, hop, N=EMU_N)


def test_dispersive_pulse_lands_on_its_group_delay(S):
    T.test_dispersive_pulse_lands_on_its_group_delay(S, N=EMU_N)
