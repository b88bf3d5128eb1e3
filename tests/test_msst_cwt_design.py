# -*- coding: utf-8 -*-
"""The design of `ssq_multi_squeeze_cwt` on the host alone (CPU): the launcher's sizing queries against the restated
rule for every row count, `row_frequencies`, the NumPy statement on its closed-form columns and against a plain
double loop, the power of the order planes over a descending table, the ABI's symbol set, and the contraction of the
first-order map of a Morlet wavelet on a linear chirp, row by row."""
import os
import re
import numpy as np
import pytest
from conftest import ROOT
import msst
import msst_cwt as M

DTYPES = ['float32', 'float64']


# ------------------------------------------------------------------------------------------ sizing, symbols
def test_tile_queries_are_the_rule():
    """`ssq_multi_squeeze_cwt_tile` and `_max_rows` (no device call) against ``160 KiB / (cols * 3 * sizeof(real) +
    8)`` for every row count in 1 .. 3000, both dtypes; the documented limits as numbers."""
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert M.LDS_BYTES == 160 * 1024 and M.TILE_COLS == (16, 8, 4) and M.REALS_PER_ROW == 3 and M.TABLE_BYTES == 8
    assert [M.tile_rows('float32', c) for c in M.TILE_COLS] == [819, 1575, 2925]
    assert [M.tile_rows('float64', c) for c in M.TILE_COLS] == [417, 819, 1575]
    for dtype, code, size in (('float32', _lib.F32, 4), ('float64', _lib.F64, 8)):
        assert lib.ssq_multi_squeeze_cwt_max_rows(code) == M.tile_rows(dtype, 4)
        seen = set()
        for rows in range(0, 3001):
            got = lib.ssq_multi_squeeze_cwt_tile(code, rows)
            assert got == M.tile(dtype, rows), (dtype, rows)
            if got:
                assert rows * (got * 3 * size + 8) <= M.LDS_BYTES            # the launch fits the LDS
                assert got == 16 or rows * (2 * got * 3 * size + 8) > M.LDS_BYTES    # ... and no wider tile would
            seen.add(got)
        assert seen == {0, 16, 8, 4}
        # the table takes rows from the linear entry's tiles, never gives any
        assert lib.ssq_multi_squeeze_cwt_max_rows(code) < lib.ssq_multi_squeeze_max_rows(code)
    assert lib.ssq_multi_squeeze_cwt_max_rows(7) == 0 and lib.ssq_multi_squeeze_cwt_tile(7, 100) == 0
    assert lib.ssq_multi_squeeze_cwt_tile(_lib.F32, -5) == 0 and lib.ssq_multi_squeeze_cwt_tile(_lib.F32, 1 << 40) == 0


def test_abi_symbol_set():
    from ssqueezepy_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'ssq_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = sorted(set(re.findall(r'\b(ssq_[a-z0-9_]+)\s*\(', txt)))
    assert sorted(_lib.EXPORTS) == declared
    assert {'ssq_multi_squeeze_cwt', 'ssq_multi_squeeze_cwt_max_rows', 'ssq_multi_squeeze_cwt_tile'} <= set(declared)
    assert _lib.ABI_VERSION >= 119 and _lib.load().ssq_version() >= 119
    import ssqueezepy_amd
    from ssqueezepy_amd import algos, wavelets
    assert ssqueezepy_amd.multi_squeeze_cwt_gpu is algos.multi_squeeze_cwt_gpu
    assert ssqueezepy_amd.row_frequencies is wavelets.row_frequencies and callable(ssqueezepy_amd.msst_cwt)


# ------------------------------------------------------------------------------------------ row_frequencies
@pytest.mark.parametrize('wavelet', ['gmw', ('morlet', {'mu': 13.4})], ids=['gmw', 'morlet'])
def test_row_frequencies(wavelet):
    import reassign_cwt as RC
    from ssqueezepy_amd import algos
    from ssqueezepy_amd.wavelets import row_frequencies, center_frequency
    wav, sc, freqs, _, _ = RC.design(wavelet, 1024)
    fr = row_frequencies(wav, sc)
    assert fr.dtype == np.float64 and fr.shape == sc.shape and (np.diff(fr) < 0).all()
    assert np.array_equal(fr, RC.row_freqs(wav, sc))
    assert np.array_equal(row_frequencies(wav, sc.reshape(-1, 1).astype(np.float32), fs=1),
                          RC.row_freqs(wav, sc.astype(np.float32)))
    assert np.array_equal(row_frequencies(wav, sc, fs=400.), center_frequency(wav, kind='peak-ct') * 400. / (2 * np.pi * sc))
    # `reassign_cwt_home` places its windows by the same frequencies
    wc = center_frequency(wav, kind='peak-ct')
    home = algos.reassign_cwt_home(sc, freqs, flipud=True, wc=wc, fs=1.)
    assert np.array_equal(home, len(sc) - 1 - algos._host_bins(fr, *RC.grid_params(freqs), len(sc) - 1))
    # what the kernel's table must be: finite, strictly monotone
    assert algos._row_table('row_freqs', fr, len(fr)) is not None
    for bad, msg in ((fr[:-1], 'one entry per row'), (np.where(np.arange(len(fr)) == 3, np.inf, fr), 'finite'),
                     (np.where(np.arange(len(fr)) == 3, fr[2], fr), 'strictly monotone')):
        with pytest.raises(ValueError, match=msg):
            algos._row_table('row_freqs', bad, len(fr))


# ------------------------------------------------------------------------------------------ the statement
def run_statement(dtype):
    def run(wcol, fr, n_iter, interp):
        w = np.asarray(wcol, dtype=dtype).reshape(1, len(fr), 1)
        return M.statement(w, fr, n_iter, interp == 'linear').reshape(-1).astype(np.float64)
    return run


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_statement_closed_forms(dtype, interp):
    M.crafted_cases(run_statement(dtype), dtype, interp)


def test_statement_half_positions_and_neighbours():
    M.half_and_neighbour_cases(run_statement('float64'))
    # NaN is skipped like inf
    fr = M.FR_DESC
    w = np.full(len(fr), np.nan)
    w[0] = fr[5]
    wf = run_statement('float64')(w, fr, 4, 'linear')
    assert wf[0] == fr[5] and np.isinf(wf[1:]).all()


def loop_statement(w, fr, n_iter, interp):
    """The definition as a plain double loop over points and passes, the interval by a linear scan."""
    B, rows, n = w.shape
    out = np.full(w.shape, np.inf)
    desc = fr[1] < fr[0]
    lo, hi = min(fr[0], fr[-1]), max(fr[0], fr[-1])
    for b in range(B):
        for c in range(n):
            col = w[b, :, c].astype(np.float64)
            for i in range(rows):
                f = col[i]
                if not np.isfinite(f):
                    continue
                for _ in range(n_iter - 1):
                    if not (lo <= f <= hi):
                        break
                    i0 = max(k for k in range(rows - 1) if (fr[k] >= f if desc else fr[k] <= f))
                    a = (f - fr[i0]) / (fr[i0 + 1] - fr[i0])
                    assert 0. <= a <= 1.
                    r = i0 + 1 if a > .5 or (a == .5 and i0 % 2 == 1) else i0
                    g = col[r]
                    if interp and np.isfinite(col[i0]) and np.isfinite(col[i0 + 1]):
                        g = col[i0] + a * (col[i0 + 1] - col[i0])
                    if not np.isfinite(g) or g == f:
                        break
                    f = g
                out[b, i, c] = f
    return out.astype(w.dtype)


@pytest.mark.parametrize('kind', M.TABLES)
def test_statement_is_the_definition(kind):
    """The vectorised statement (`np.searchsorted`) against the double loop, on every kind of table, both dtypes."""
    rows = 33
    fr, metric = M.table(kind, rows)
    for dtype in DTYPES:
        _, w = M.planes(1, rows, 7, dtype, fr, metric)
        for interp in (False, True):
            for n_iter in (1, 2, 6):
                a, b = M.statement(w, fr, n_iter, interp), loop_statement(w, fr, n_iter, interp)
                assert np.array_equal(a, b), (kind, dtype, interp, n_iter)
    assert (M.statement(w, fr, 6, True) != M.statement(w, fr, 1, True)).any()


def test_tables_are_what_they_claim():
    for kind in M.TABLES:
        for rows in (2, 33, 245):
            fr, _ = M.table(kind, rows)
            d = np.diff(fr)
            assert len(fr) == rows and np.isfinite(fr).all() and (fr > 0).all()
            assert (d > 0).all() if kind == 'linear-ascending' else (d < 0).all(), (kind, rows)
            assert max(fr[0], fr[-1]) / min(fr[0], fr[-1]) <= 2. ** 16
    lp = M.table('log-piecewise', 245)[0]
    from ssqueezepy_amd.scales import infer_scaletype
    assert infer_scaletype(1. / lp)[0] == 'log-piecewise'                  # the library's own two-piece table
    assert infer_scaletype(1. / M.table('log', 245)[0])[0] == 'log'
    assert infer_scaletype(1. / M.table('hyperbolic', 245)[0])[0] == 'linear'
    with pytest.raises(ValueError):
        infer_scaletype(1. / M.table('irregular', 245)[0])                # no closed form describes it
    for rows in (16, 33, 245, 819, 2925):
        fr = M.table('irregular', rows)[0]
        kinds = [infer_scaletype(M.bin_grid(g, fr))[0] for g in M.GRIDS]
        assert kinds == M.GRIDS, (rows, kinds)


def test_which_tables_take_the_closed_form_guess():
    """The entry's first guess, restated (`msst_cwt.hint_fit`): kept on the geometric tables, one piece or two, where it
    names the right row or a neighbour; dropped on the hyperbolic and the irregular one, which go to the search; kept
    on the jittered one, whose test planes then reach every arm -- the row itself, one below, one above, and two off,
    which goes to the search after all. Whatever the guess, the bits are the search's: the GPU module compares every
    one of these tables with the statement."""
    for kind, rows in (('log', 40), ('log', 300), ('log', 2925), ('log-piecewise', 33), ('log-piecewise', 245)):
        fr = M.table(kind, rows)[0]
        h = M.hint_fit(fr)
        assert h is not None, (kind, rows)
        f = np.exp(np.random.default_rng(0).uniform(np.log(fr[-1]), np.log(fr[0]), 20000))
        off = M.hint_guess(h, f) - M.interval(fr, f)
        assert np.abs(off).max() <= 1 and (off == 0).mean() > .99, (kind, rows)
    for kind, rows in (('hyperbolic', 40), ('irregular', 40), ('irregular', 131), ('linear-ascending', 40)):
        assert M.hint_fit(M.table(kind, rows)[0]) is None, (kind, rows)
    assert M.hint_fit(np.array([3., 2., 1., -1.])) is None and M.hint_fit(np.array([3., 2., 1.])) is None
    fr, metric = M.table('jittered', 131)
    h = M.hint_fit(fr)
    assert h is not None
    w = M.planes(1, 131, 7, 'float64', fr, metric)[1]
    f = w[np.isfinite(w) & (w >= fr[-1]) & (w <= fr[0])]
    off = M.hint_guess(h, f) - M.interval(fr, f)
    assert {-1, 0, 1, 2} <= set(np.unique(off).tolist())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['one_bin', 'two_bins'])
def test_order_planes_over_a_descending_table(name, dtype):
    Sx, w, fr, Sfs, n_iter, bins, f_final = M.order_case(name, dtype)
    assert (np.diff(fr) < 0).all() and np.array_equal(Sfs[bins], f_final)
    for interp in (False, True):
        wf = M.statement(w, fr, n_iter, interp)
        assert np.array_equal(wf[0, :, 0].astype(np.float64), f_final)
    assert len(np.unique(bins)) == (1 if name == 'one_bin' else 2)
    fwd, rev = msst.ordered_sum(Sx, bins, 1.), msst.ordered_sum(Sx, bins, 1., reverse=True)
    assert np.isfinite(fwd.view(Sx.real.dtype)).all() and (fwd != rev).any()


# ------------------------------------------------------------------------------------------ why it works
def test_contraction_row_by_row_on_a_morlet_chirp():
    """A Morlet row at scale `a` is a Gaussian-window STFT of width ``a`` samples read at ``mu / (2 pi a)``: on a linear
    chirp of rate `c` the first-order map is ``w = phi' + kappa_a (fr_a - phi')`` with ``kappa_a = A^2 / (1 + A^2)``,
    ``A = 2 pi c a^2`` -- a contraction towards the instantaneous frequency in every row, stronger in the upper rows.
    Checked on the NumPy planes in the ridge's rows (``|W| >= 0.3`` of the column's maximum) of the interior columns;
    iterating then closes in: the statement's error after `m` passes falls with `m`."""
    import reassign_cwt as RC
    from ssqueezepy_amd.padding import pad_geometry
    from ssqueezepy_amd.wavelets import row_frequencies
    N, mu = 512, 13.4
    x, f = M.signal('chirp', N)
    wav, sc, _, _, _ = RC.design(('morlet', {'mu': mu}), N)
    Mp, n1, _ = pad_geometry(N)
    W, dW = RC.np_cwt(x, wav.fn, sc, Mp, n1), RC.np_cwt(x, wav.fn, sc, Mp, n1, deriv=True)
    with np.errstate(all='ignore'):
        w = np.abs(np.imag(dW / W)) / (2 * np.pi)
    fr = row_frequencies(wav, sc)
    cols = np.arange(N // 4, 3 * N // 4)
    A = np.abs(W)
    ridge = A[:, cols] >= .3 * A[:, cols].max(axis=0)
    e0 = np.abs(fr[:, None] - f[None, cols])
    e1 = np.abs(w[:, cols] - f[None, cols])
    spacing = np.abs(np.gradient(fr))[:, None]
    sel = ridge & (e0 >= spacing)                       # (a row on the ridge itself has nothing to contract)
    assert sel.sum() > 2000
    ratio = (e1 / e0)[sel]
    a = mu / (2 * np.pi * np.broadcast_to(fr[:, None], e0.shape)[sel])
    Ak = 2 * np.pi * (.3 / N) * a * a
    kappa = Ak * Ak / (1. + Ak * Ak)
    assert ratio.max() < .75 and np.abs(ratio - kappa).max() < 1e-6
    assert kappa.min() < .05 and kappa.max() > .5       # the factor depends on the row
    # the iteration: the energy-weighted error of the ridge's rows falls pass by pass
    wr = np.where(A >= 1e-8 * A.max(), w, np.inf)
    errs = []
    for m in (1, 2, 5, 10):
        wf = M.statement(wr[None], fr, m, True)[0][:, cols]
        errs.append(float((np.abs(wf - f[None, cols]) * A[:, cols] ** 2)[ridge].sum() / (A[:, cols] ** 2)[ridge].sum()))
    assert errs[0] > errs[1] > errs[2] > errs[3] and errs[3] < .05 * errs[0], errs
