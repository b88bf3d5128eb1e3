# -*- coding: utf-8 -*-
"""The design of `ssq_multi_squeeze` without the library (CPU): the NumPy statement on its closed-form cases, the
contraction of the first-order map of a Gaussian-window chirp, the order planes' power to tell two orders of addition
apart, and the launcher's sizing against the LDS."""
import numpy as np
import pytest
import msst

DTYPES = ['float32', 'float64']
ROWS, F0, DF = 24, 2., .5


def at(k):
    return F0 + DF * np.asarray(k, dtype=np.float64)


def column(wcol, n_iter, interp, dtype='float64'):
    w = np.asarray(wcol, dtype=dtype).reshape(1, ROWS, 1)
    return msst.statement(w, F0, DF, n_iter, interp).reshape(-1).astype(np.float64)


@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_statement_closed_forms(dtype, interp):
    i = np.arange(ROWS)
    inf = np.inf
    for m in (1, 2, 5, ROWS + 3):                                # w[i] = Sfs[i + 1]: m passes climb m rows, then leave
        assert np.array_equal(column(at(i + 1), m, interp, dtype), at(np.minimum(i + m, ROWS)))
    w = np.full(ROWS, inf)                                       # a two-cycle
    w[3], w[9] = at(9), at(3)
    for m in (1, 2, 3, 10, 11):
        wf = column(w, m, interp, dtype)
        assert (wf[3], wf[9]) == ((at(9), at(3)) if m % 2 else (at(3), at(9)))
    w = at(i - np.where(i % 3 == 0, 0, 1))                       # fixed points
    assert np.array_equal(column(w, 3, interp, dtype), at(i - i % 3))
    assert np.array_equal(column(w, 1024, interp, dtype), at(i - i % 3))
    w = np.full(ROWS, inf)                                       # a chain into a row that holds nothing
    w[:4] = at([1, 2, 3, 4])
    assert np.array_equal(column(w, 10, interp, dtype)[:4], at([4] * 4))
    w = np.full(ROWS, inf)                                       # chains that leave the grid, above and below
    w[:3] = at([1, 2, ROWS + 6.25])
    w[5], w[6] = at(6), at(-3.5)
    wf = column(w, 10, interp, dtype)
    assert np.array_equal(wf[:3], at([ROWS + 6.25] * 3)) and np.array_equal(wf[5:7], at([-3.5] * 2))
    w = np.full(ROWS, np.nan)                                    # NaN is skipped like inf
    w[0] = at(5)
    wf = column(w, 4, interp, dtype)
    assert wf[0] == at(5) and np.isinf(wf[1:]).all()


def test_statement_rounding_and_neighbours():
    inf = np.inf
    w = np.full(ROWS, inf)
    w[0], w[1], w[2], w[4] = at(2.5), at(3.5), at(20), at(21)    # half to even: 2.5 -> 2, 3.5 -> 4
    wf = column(w, 2, False)
    assert (wf[0], wf[1]) == (at(20), at(21))
    w = np.full(ROWS, inf)
    w[0], w[1], w[2] = at(10.25), at(12.25), at(12.75)
    w[10], w[11], w[12] = at(4), at(8), at(16)
    wf = column(w, 2, True)
    assert wf[0] == at(4) + .25 * (at(8) - at(4)) and wf[1] == at(16) and wf[2] == at(12.75)


def test_contraction_on_a_gaussian_window_chirp():
    """A linear chirp of rate `c` Hz/s seen through the window exp(-tau^2 / (2 sigma^2)): the first-order estimate is
    ``w(f) = phi' + kappa (f - phi')`` with ``kappa = a^2 / (1 + a^2)``, ``a = 2 pi c sigma^2`` -- a contraction
    towards the instantaneous frequency phi'. The real-valued iteration shrinks every point's error by `kappa` per
    pass (linear interpolation of a linear map is exact); the nearest-row form stalls within half a row."""
    fs, n_fft = msst.FS, msst.N_FFT
    c, sigma = 400., (n_fft / 8.) / fs
    a = 2 * np.pi * c * sigma * sigma
    kappa = a * a / (1. + a * a)
    assert .85 < kappa < .87
    Sfs = np.linspace(0, .5 * fs, n_fft // 2 + 1)
    f0, df = msst.row_grid(Sfs)
    phi = 251.3                                                  # between two rows
    w = (phi + kappa * (Sfs - phi)).reshape(1, -1, 1)
    err0 = Sfs - phi
    for m in (1, 2, 5, 10, 20):
        wf = msst.statement(w, f0, df, m, True).reshape(-1)
        assert np.abs((wf - phi) - kappa ** m * err0).max() <= 1e-9 * np.abs(err0).max(), m
    near = msst.statement(w, f0, df, 200, False).reshape(-1)
    stalled = np.abs(near - phi)
    # a row moves on only while kappa |f - phi| lies more than half a row from it: the integer form keeps an error of
    # up to kappa / (1 - kappa) / 2 rows, here about 3
    assert stalled.max() > df and stalled.max() <= kappa / (1. - kappa) * df
    assert np.abs(msst.statement(w, f0, df, 200, True).reshape(-1) - phi).max() < 1e-9


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['one_bin', 'two_bins'])
def test_order_planes_tell_the_orders_apart(name, dtype):
    Sx, w, Sfs, n_iter, final = msst.order_planes(dtype)[name]
    f0, df = msst.row_grid(Sfs)
    for interp in (False, True):
        wf = msst.statement(w, f0, df, n_iter, interp)
        assert np.array_equal(wf[0, :, 0].astype(np.float64), Sfs[final].astype(np.float64))
    assert len(np.unique(final)) == (1 if name == 'one_bin' else 2)
    fwd, rev = msst.ordered_sum(Sx, final, 1.), msst.ordered_sum(Sx, final, 1., reverse=True)
    assert np.isfinite(fwd.view(Sx.real.dtype)).all() and (fwd != rev).any()


def test_sizing_against_the_lds():
    assert msst.LDS_BYTES == 160 * 1024 and msst.TILE_COLS == (16, 8, 4) and msst.REALS_PER_ROW == 3
    for dtype, size in (('float32', 4), ('float64', 8)):
        rows = [msst.tile_rows(dtype, cols) for cols in msst.TILE_COLS]
        assert rows[0] < rows[1] < rows[2] and rows[2] >= 1025           # n_fft = 2048 fits the narrowest tile
        for cols, r in zip(msst.TILE_COLS, rows):
            assert r * cols * 3 * size <= msst.LDS_BYTES < (r + 1) * cols * 3 * size
    assert msst.tile_rows('float32', 4) == 3413 and msst.tile_rows('float64', 4) == 1706
    # LDS per row: 1.5 times the accumulate tile's complex cell
    assert msst.REALS_PER_ROW / 2 == 1.5
