# -*- coding: utf-8 -*-
"""The long-signal tests of tests/test_gpu_long_signals.py with the product's own kernels and host
code under the CPU emulator (tests/emu/, tests/emu_backend.py), run as they are: `cwt` with its
derivative at all four lengths (M = 2^19 .. 2^22: the host dispatch, the slots and the twiddle tables
of every LDS FFT length, the 1024- and 2048-point ones included) with the per-row bound on the exact
rows, the batch of two at M = 2^20, and the fused form at the shortest length, once, with `dWx` (one
emulated run of the tile kernel takes ~15 s there and minutes at M = 2^22; the lean run is the GPU
module's). CPU-only."""
import pytest
import emu_backend
import test_gpu_long_signals as T


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    T._CASE.clear()
    with emu_backend.emulated() as mod:
        yield mod
    T._CASE.clear()


@pytest.fixture(scope='module', params=T.NS)
def case(request, orc):
    yield T.make_case(orc, request.param)
    T._CASE.clear()


@pytest.mark.parametrize('ext', ['1', '0'])
def test_cwt_rows_vs_float64_statement(S, orc, case, ext, monkeypatch):
    T.check_cwt_rows(S, orc, case, ext, monkeypatch)


def test_long_batch_equals_single(S, monkeypatch):
    T.test_long_batch_equals_single(S, monkeypatch)


def test_ssq_cwt_long_vs_oracle(S, orc):
    T.check_ssq_cwt_long(S, orc, T.make_case(orc, T.NS[0]), lean=False)


def test_no_tile_class_has_a_2048_point_factor():
    T.test_no_tile_class_has_a_2048_point_factor()
