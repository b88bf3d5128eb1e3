# -*- coding: utf-8 -*-
"""The row-count tests of tests/test_gpu_tile_rows.py with the product's own kernels and host code under the CPU
emulator (tests/emu/, tests/emu_backend.py), run as they are on a subset: one signal per call, N = 4201; the
kernel by row count at 319 (pair kernel's last), 320, 384 (a multiple of the write-out round), 511 and 512 rows
by default and at 320 rows in the ordered mode; four of the float64-tile builds; the 16-column kernel's bins at
320 rows. The emulator runs work-items as host threads: it checks the kernels' logic and the host's routing,
not the device's LDS atomics, unaligned stores or scalar-register handling -- those are the GPU module's.
CPU-only."""
import pytest
import emu_backend
import test_gpu_tile_rows as T

N = 4201


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    T._CASE.clear()
    with emu_backend.emulated() as mod:
        yield mod
    T._CASE.clear()


def test_row_limits_are_the_documented_ones():
    T.test_row_limits_are_the_documented_ones()


@pytest.mark.parametrize('na,mode', [(319, 'f64'), (320, 'f64'), (384, 'f64'), (511, 'f64'), (512, 'f64'),
                                     (320, 'ordered')])
def test_tile_kernel_by_row_count(S, orc, na, mode, monkeypatch):
    monkeypatch.setenv('SSQ_TILE_ORDER', mode)
    monkeypatch.delenv('SSQ_DEBUG_TILE_PAIR', raising=False)
    T.check_rows(S, orc, N, na, nsig=1)


@pytest.mark.parametrize('na,grid,weights', [(511, 'log-piecewise', 'vec64'), (320, 'linear', 'vec32')])
def test_16_column_tile_every_build(S, orc, na, grid, weights, monkeypatch):
    monkeypatch.delenv('SSQ_TILE_ORDER', raising=False)
    monkeypatch.delenv('SSQ_DEBUG_TILE_PAIR', raising=False)
    T.check_build(S, orc, N, na, grid, weights, nsig=1)


def test_single_column_32_tile_every_build(S, orc, monkeypatch):
    monkeypatch.delenv('SSQ_TILE_ORDER', raising=False)
    monkeypatch.setenv('SSQ_DEBUG_TILE_PAIR', '0')
    T.check_build(S, orc, N, 319, 'linear', 'vec64', pair=False, nsig=1)


@pytest.mark.parametrize('weights', ['scalar', 'vec64'])
def test_16_column_bins_are_the_oracles_integers(S, orc, weights, monkeypatch):
    monkeypatch.delenv('SSQ_TILE_ORDER', raising=False)
    monkeypatch.delenv('SSQ_DEBUG_TILE_PAIR', raising=False)
    T.check_bins(S, orc, N, 320, weights, nsig=1)
