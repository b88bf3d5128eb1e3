# -*- coding: utf-8 -*-
"""The checks of tests/test_gpu_reassign_rows.py with the product's own kernels and host code under the CPU emulator
(tests/emu/, tests/emu_backend.py), on a subset: one row count on each side of every LDS edge with few columns and one
grid and weight kind per bin source, n = 1, TC + 1, 8 TC + 1 on every build, all crafted maps on every build (at its first row count), the
`exact_sum` bounds of the unordered tile, `out=` and the refusals. The emulator runs work-items as fibers in a fixed
order: it checks the kernels' logic and the host's routing, not the device's LDS atomics or DPP moves -- those are the
GPU module's. CPU-only."""
import pytest
import emu_backend
import reassign_rows as R
import test_gpu_reassign_rows as T


@pytest.fixture(scope='module')
def A():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated():
        from ssqueezepy_amd import algos
        yield algos


EDGES = [(d, na) for d in T.DTYPES for e in sorted(set(R.ORDERED_LIMITS[d] + R.F64_LIMITS[d])) for na in (e, e + 1)]


@pytest.mark.parametrize('dtype,na', EDGES)
def test_every_route_by_row_count(A, orc, dtype, na, monkeypatch):
    i = EDGES.index((dtype, na))
    T.check_rows(A, orc, dtype, na, monkeypatch, n=R.columns_for(na), grids=(R.GRIDS[i % 3],), weights=(R.WEIGHTS[i % 3],))


@pytest.mark.parametrize('dtype,kernel,cols', T.BUILD_IDS)
def test_column_count_on_every_build(A, orc, dtype, kernel, cols, monkeypatch):
    TC = 256 if kernel == 'global' else cols
    T.check_columns(A, orc, dtype, kernel, cols, monkeypatch, ns=(1, TC + 1) + ((8 * TC + 1,) if kernel != 'global' else ()))


@pytest.mark.parametrize('dtype,cols', list(R.F64_BUILDS))
def test_column_count_on_the_unordered_tile(A, orc, dtype, cols, monkeypatch):
    T.check_f64_columns(A, orc, dtype, cols, monkeypatch, ns=(1, cols + 1, 8 * cols + 1))


@pytest.mark.parametrize('dtype,kernel,cols', T.BUILD_IDS)
def test_crafted_maps_on_every_build(A, orc, dtype, kernel, cols, monkeypatch):
    # (the first row count of the build, past four steps of it: the emulation's cost grows with the rows)
    T.check_patterns(A, orc, dtype, kernel, cols, monkeypatch, n=cols + 1 if kernel != 'global' else 3,
                     na=max(T.first_rows(dtype, kernel, cols), 100))


@pytest.mark.parametrize('dtype,cols', list(R.F64_BUILDS))
def test_unordered_tile_against_the_exact_sum(A, orc, dtype, cols, monkeypatch):
    T.check_f64_kernel(A, orc, dtype, cols, monkeypatch, n=cols + 1)


@pytest.mark.parametrize('dtype,na', [('float32', 320), ('float32', 2561), ('float32', 5121), ('float64', 640),
                                      ('float64', 1280), ('float64', 2561)])
def test_out_is_fully_overwritten(A, orc, dtype, na, monkeypatch):
    T.check_out(A, orc, dtype, na, monkeypatch, n=5)


def test_indexed_sum_bins_refuses(A, monkeypatch):
    monkeypatch.delenv('SSQ_TILE_ORDER', raising=False)
    T.check_refusals(A)
