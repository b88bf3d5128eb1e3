# -*- coding: utf-8 -*-
"""What the tests of `ssq_multi_squeeze_cwt` share (tests/test_gpu_msst_cwt.py, its emulated twin and
tests/test_msst_cwt_design.py): the NumPy statement of the iteration on a table of rows (include/ssq_hip.h, DESIGN.md
section 4.5.11), the launcher's sizing restated, the tables, the seeded planes, the signals, and a NumPy float64
restatement of the whole transform.

As in tests/msst.py the statement works on separate float64 arrays with one ufunc per operation and a Python loop over
the iterations; the interval `i0` comes from `np.searchsorted`, which, like the entry's definition, compares against the
table alone. It returns `w_final` rounded to the dtype. The expected `Tx` is then `indexed_sum_onfly(Wx, w_final, ...)`
on the same grid: that entry is pinned to the oracle and ordered, so it states the binning (the device's own `log2`
included) and the accumulation, summation order included.
"""
import numpy as np
from msst import _np, EPS, LDS_BYTES, TILE_COLS, REALS_PER_ROW, order_planes  # noqa: F401

TABLE_BYTES = 8                 # LDS per row on top of the slabs: the rows' table, float64
TABLES = ['log', 'log-piecewise', 'hyperbolic', 'linear-ascending', 'irregular', 'jittered']
GRIDS = ['linear', 'log', 'log-piecewise']


# ------------------------------------------------------------------------------------------ sizing
def tile_rows(dtype, cols):
    """The most rows a tile of `cols` columns holds next to the table: 160 KiB / (cols * 3 * sizeof(real) + 8)."""
    return LDS_BYTES // (cols * REALS_PER_ROW * np.dtype(dtype).itemsize + TABLE_BYTES)


def tile(dtype, rows):
    """The columns of the tile the launcher takes, the widest that fits; 0 = refused."""
    if rows < 2:
        return 0
    for cols in TILE_COLS:
        if rows <= tile_rows(dtype, cols):
            return cols
    return 0


# ------------------------------------------------------------------------------------------ the statement
def interval(fr, f):
    """`i0` for every `f` inside the table's range: the largest ``i <= rows - 2`` with ``fr[i] >= f`` (descending
    table; ``fr[i] <= f`` for an ascending one)."""
    rows = len(fr)
    if fr[1] < fr[0]:
        # asc[j] = fr[rows - 1 - j]: the smallest j >= 1 with asc[j] >= f
        j = np.clip(np.searchsorted(fr[::-1], f, side='left'), 1, rows - 1)
        return rows - 1 - j
    return np.clip(np.searchsorted(fr, f, side='right') - 1, 0, rows - 2)


def statement(w, fr, n_iter, interp):
    """`w_final` of the dtype of `w` (B, rows, n): the entry's iteration, ``inf`` where ``w`` is not finite."""
    W = np.asarray(w).astype(np.float64)
    fr = np.asarray(fr, dtype=np.float64).reshape(-1)
    assert W.shape[1] == len(fr)
    lo, hi = min(fr[0], fr[-1]), max(fr[0], fr[-1])
    have = np.isfinite(W)
    f, moving = W.copy(), have.copy()
    with np.errstate(all='ignore'):
        for _ in range(int(n_iter) - 1):
            if not moving.any():
                break
            inside = moving & (f >= lo) & (f <= hi)                       # (false for NaN)
            fi = np.where(inside, f, fr[0])
            i0 = interval(fr, fi)
            t0 = fr[i0]
            a = np.divide(np.subtract(fi, t0), np.subtract(fr[i0 + 1], t0))
            r = i0 + ((a > .5) | ((a == .5) & (i0 % 2 == 1)))             # half to the even row
            g = np.take_along_axis(W, r, axis=1)
            if interp:
                wa, wc = np.take_along_axis(W, i0, axis=1), np.take_along_axis(W, i0 + 1, axis=1)
                lerp = np.add(wa, np.multiply(a, np.subtract(wc, wa)))
                g = np.where(np.isfinite(wa) & np.isfinite(wc), lerp, g)
            ok = inside & np.isfinite(g)
            moving = ok & (g != f)
            f = np.where(ok, g, f)
    return np.where(have, f, np.inf).astype(np.asarray(w).dtype)


# ------------------------------------------------------------------------------------------ the entry's first guess
def hint_fit(fr):
    """The closed-form first guess the entry fits to a table (`msst_fit_hint`, csrc/ssq_multi_squeeze.inl), restated:
    two geometric pieces that meet at the row where ``log2(fr)`` bends most, each through its end rows, in float32;
    None where the guess is further than one row from the right one at some row's frequency or between two rows."""
    f32 = np.float32
    fr = np.asarray(fr, dtype=np.float64)
    rows = len(fr)
    if rows < 4 or not (fr > 0).all():
        return None
    lg = np.log2(fr)
    s = int(np.argmax(np.abs(lg[2:] - 2 * lg[1:-1] + lg[:-2]))) + 1
    h = dict(seam=fr[s], l0=(f32(lg[0]), f32(lg[s])), row0=(f32(0), f32(s)), rows=rows, desc=bool(fr[1] < fr[0]),
             slope=(f32(s / (lg[s] - lg[0])), f32((rows - 1 - s) / (lg[-1] - lg[s]))))
    i = np.arange(rows - 1)
    for f in (fr[:-1], np.sqrt(fr[:-1] * fr[1:])):
        if (np.abs(hint_guess(h, f) - i) > 1).any():
            return None
    return h


def hint_guess(h, f):
    f = np.asarray(f, dtype=np.float64)
    p = np.where((f >= h['seam']) if h['desc'] else (f <= h['seam']), 0, 1)
    l0, slope, row0 = (np.asarray(h[k], dtype=np.float32)[p] for k in ('l0', 'slope', 'row0'))
    pos = (row0 + (np.log2(f.astype(np.float32)) - l0) * slope).astype(np.float32)
    return np.clip(np.floor(pos), 0, h['rows'] - 2).astype(np.int64)


# ------------------------------------------------------------------------------------------ tables, grids, planes
def table(kind, rows, seed=0):
    """``(fr, metric)``: a table of `rows` centre frequencies, float64, and the metric its rows are spread in ('log' or
    'linear'; `planes` draws `w` uniformly in it).
      'log'               descending geometric, 32 voices (more beyond 256 rows, so that the table spans 8 octaves at
                          the most): `ssq_cwt`'s rows on 'log' scales
      'log-piecewise'     the library's own: `row_frequencies` of the scales `_ssq_design` makes for a gmw wavelet with
                          4 voices (33 rows) or 32 (245 rows), the last `rows` of them
      'hyperbolic'        c / scales on linear scales
      'linear-ascending'  rows + i / 2
      'irregular'         descending over 8 octaves in seeded steps, the largest ten times the smallest: no closed form
                          finds a row in it
      'jittered'          descending, 32 voices, every row off its place by a seeded +-0.45 rows in the first half and
                          by up to 1.45 rows in a block of the second: geometric enough for the entry's closed-form
                          guess to be kept (`hint_fit`), and wrong enough for it to be off by -1, 1 and 2 rows"""
    i = np.arange(rows, dtype=np.float64)
    if kind == 'log':
        return .4 * 2. ** (-i / max(32., rows / 8.)), 'log'
    if kind == 'log-piecewise':
        return library_table(rows), 'log'
    if kind == 'hyperbolic':
        return 60. / (3. + i), 'log'
    if kind == 'linear-ascending':
        return rows + i / 2., 'linear'
    if kind == 'jittered':
        rng = np.random.default_rng([seed, rows, 5])
        u = rng.uniform(-.45, .45, rows)
        u[0] = u[-1] = 0.
        h = rows // 2
        u = np.where(i >= h, 1.45 * np.clip(np.minimum(i - h, rows - 4 - i) / 2., 0., 1.), u)
        return .4 * 2. ** (-(i + u) / 32.), 'log'
    rng = np.random.default_rng([seed, rows, 77])
    steps = rng.uniform(.1, 1., rows)
    return 40. * 2. ** (-np.cumsum(steps) * (8. / steps.sum())), 'log'


_LIB_TABLES = {}


def library_table(rows):
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    from ssqueezepy_amd.wavelets import row_frequencies
    if not _LIB_TABLES:
        for N, nv in ((512, 4), (2048, 32)):                    # 33 and 245 rows
            wav = make_wavelet('gmw', N, 'float64')
            sc = _ssq_design(wav, 'log-piecewise', nv, N, 1., None, 'peak', True)[0]
            _LIB_TABLES[len(sc)] = row_frequencies(wav, sc)
    for have in sorted(_LIB_TABLES):
        if have >= rows:
            # the last rows: the seam of the two pieces lies in the upper scales
            return _LIB_TABLES[have][-rows:].copy()
    raise ValueError("no library table of %d rows" % rows)


def bin_grid(kind, fr):
    """`rows` bins over the table's range, float64, ascending: linear, exponential, or exponential in two pieces (the
    lower half of the rows over the lowest quarter of the log range)."""
    rows = len(fr)
    lo, hi = float(min(fr[0], fr[-1])), float(max(fr[0], fr[-1]))
    if kind == 'linear':
        return np.linspace(lo, hi, rows)
    l0, l1 = np.log2(lo), np.log2(hi)
    if kind == 'log':
        return 2. ** np.linspace(l0, l1, rows)
    r0 = rows // 2 + 1
    mid = l0 + .25 * (l1 - l0)
    return 2. ** np.concatenate([np.linspace(l0, mid, r0, endpoint=False), np.linspace(mid, l1, rows - r0)])


def grids_for(rows):
    """The bin grids a row count can tell apart: two pieces need rows enough to show one clean change of rate."""
    return GRIDS if rows >= 16 else GRIDS[:2]


def planes(B, rows, n, dtype, fr, metric, seed=0):
    """Seeded `Wx` (standard normal) and `w`: uniform, in the table's metric, over 1.5 times its range (a quarter
    below, a quarter above: some points leave the table), a quarter of the points ``inf``, three of them NaN."""
    rng = np.random.default_rng([seed, B, rows, n, 2019])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    Wx = (rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))).astype(cdt)
    lo, hi = float(min(fr[0], fr[-1])), float(max(fr[0], fr[-1]))
    u = rng.uniform(-.25, 1.25, (B, rows, n))
    if metric == 'log':
        w = np.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * u)
    else:
        w = lo + (hi - lo) * u
    w = w.astype(dtype)
    w[rng.uniform(size=w.shape) < .25] = np.inf
    flat = w.reshape(-1)
    flat[rng.choice(flat.size, size=min(3, flat.size // 4), replace=False)] = np.nan
    return Wx, w


# ------------------------------------------------------------------------------------------ crafted columns, order
ROWS_C = 24
FR_DESC = 2. ** (6 - np.arange(ROWS_C) / 4.)            # descending, geometric: 64 down to 2^0.25
FR_DYADIC = 16. - .5 * np.arange(ROWS_C)                # descending, dyadic: midpoints are exact


def rounded(fr, dtype):
    """A table whose values survive the dtype: a float32 `w` can then hold a row's frequency exactly."""
    return np.asarray(fr).astype(dtype).astype(np.float64)


def crafted_cases(run, dtype, interp):
    """The closed forms of the issue's list, through `run(wcol, fr, n_iter, interp) -> wf`; shared with the CPU module,
    which runs them on the statement."""
    inf = np.inf
    fr = rounded(FR_DESC, dtype)
    rows = len(fr)
    i = np.arange(rows)
    # every row points at fr[k] and row k holds fr[k]: after one pass the whole column sits at fr[k]
    for k in (0, 7, rows - 1):
        wf = run(np.full(rows, fr[k]), fr, 2, interp)
        assert np.array_equal(wf, np.full(rows, fr[k])), k
        assert np.array_equal(run(np.full(rows, fr[k]), fr, 1024, interp), wf)
    # f equal to a table value, both ends included (a = 0 at fr[0], a = 1 at fr[rows - 1]): row i holds fr[perm[i]]
    perm = (7 * i + 3) % rows
    wf = run(fr[perm], fr, 2, interp)
    assert np.array_equal(wf, fr[perm[perm]])
    assert 0 in perm and rows - 1 in perm
    # a two-cycle between rows 3 and 9 runs to n_iter exactly: the parity decides
    w = np.full(rows, inf)
    w[3], w[9] = fr[9], fr[3]
    for m in (1, 2, 3, 10, 11, 1024):
        wf = run(w, fr, m, interp)
        assert (wf[3], wf[9]) == ((fr[9], fr[3]) if m % 2 else (fr[3], fr[9])), m
        assert np.isinf(np.delete(wf, [3, 9])).all()
    # walks that leave the range on either side stop there: 0 -> 1 -> 2 -> above fr[0]; 5 -> 6 -> below fr[rows - 1]
    above, below = float(np.asarray(2 * fr[0]).astype(dtype)), float(np.asarray(.5 * fr[-1]).astype(dtype))
    w = np.full(rows, inf)
    w[:3] = [fr[1], fr[2], above]
    w[5], w[6] = fr[6], below
    wf = run(w, fr, 10, interp)
    assert np.array_equal(wf[:3], [above] * 3) and np.array_equal(wf[5:7], [below] * 2)
    # a chain into an inf row stops in front of it
    w = np.full(rows, inf)
    w[:4] = fr[[1, 2, 3, 4]]
    assert np.array_equal(run(w, fr, 10, interp)[:4], fr[[4] * 4])


def half_and_neighbour_cases(run):
    inf = np.inf
    fr = FR_DYADIC
    rows = len(fr)
    mid = lambda k: .5 * (fr[k] + fr[k + 1])        # noqa: E731  (exact: a == 0.5)
    # nearest: a == 0.5 goes to the even row -- between rows 2 and 3 to row 2, between rows 3 and 4 to row 4
    w = np.full(rows, inf)
    w[0], w[1], w[2], w[4] = mid(2), mid(3), fr[20], fr[21]
    wf = run(w, fr, 2, 'nearest')
    assert (wf[0], wf[1]) == (fr[20], fr[21])
    # linear: both neighbours finite -> interpolated; one inf -> the nearest row; the nearest row inf -> stays
    q = lambda k, a: fr[k] + a * (fr[k + 1] - fr[k])        # noqa: E731
    w = np.full(rows, inf)
    w[0], w[1], w[2] = q(10, .25), q(12, .25), q(12, .75)
    w[10], w[11], w[12] = fr[4], fr[8], fr[16]
    wf = run(w, fr, 2, 'linear')
    assert wf[0] == fr[4] + .25 * (fr[8] - fr[4])                # between rows 10 and 11
    assert wf[1] == fr[16]                                       # row 13 holds nothing: the nearest row, 12
    assert wf[2] == q(12, .75)                                   # the nearest row, 13, holds nothing: stop


def order_case(name, dtype):
    """The order planes of tests/msst.py over a descending table: ``fr = Sfs[::-1]``, so row `i` still walks two rows
    per pass towards the target of its parity. Returns ``(Sx, w, fr, Sfs, n_iter, bins, f_final)``: `bins` the bin every
    row ends in on the grid `Sfs`, `f_final` its final frequency."""
    Sx, w, Sfs, n_iter, final = order_planes(dtype)[name]
    Sfs64 = Sfs.astype(np.float64)
    rows = len(Sfs64)
    fr = Sfs64[::-1].copy()
    nxt = np.rint((w[0, :, 0].astype(np.float64) - 2.) * 2.).astype(int)         # Sfs = 2 + i / 2
    wd = np.ascontiguousarray(np.broadcast_to(fr[nxt][None, :, None], w.shape)).astype(dtype)
    return Sx, wd, fr, Sfs64, n_iter, rows - 1 - final, fr[final]


# ------------------------------------------------------------------------------------------ the whole transform
SIGNALS = {'fm_gmw': ('fm', 2048, 'gmw'), 'fm_morlet': ('fm', 2048, ('morlet', {'mu': 13.4})),
           'chirp_gmw': ('chirp', 512, 'gmw')}
PASSES = [(1, 'linear'), (2, 'linear'), (5, 'linear'), (10, 'linear'), (10, 'nearest')]


def make_wavelet(wavelet, N, dtype):
    """The wavelet as the transforms make it from a name (`reassign_cwt.design` does the same in float64)."""
    from ssqueezepy_amd import Wavelet
    from ssqueezepy_amd._cwt import _process_gmw_wavelet
    if isinstance(wavelet, tuple):
        wavelet = (wavelet[0], dict(wavelet[1]))
    return Wavelet(_process_gmw_wavelet(wavelet, True), N=N, dtype=dtype)


def signal(kind, N):
    """(x, instantaneous frequency in cycles per sample): the FM tone ``0.15 + 0.05 cos(2 pi t / 300)`` or the linear
    chirp 0.05 -> 0.35 over `N` samples."""
    t = np.arange(N, dtype=np.float64)
    if kind == 'fm':
        f = .15 + .05 * np.cos(2 * np.pi * t / 300.)
        ph = .15 * t + .05 * 300. / (2 * np.pi) * np.sin(2 * np.pi * t / 300.)
    else:
        f = .05 + .3 * t / N
        ph = .05 * t + .15 * t * t / N
    return np.cos(2 * np.pi * ph), f


def share(Tx, f_true, freqs_out):
    """The share of ``|Tx|^2``, over the interior three quarters of the columns, within +-1 bin of the bin of
    `freqs_out` (the order the transform returns) nearest to the true frequency in log-frequency."""
    import reassign_cwt as RC
    return RC.ridge_share(np.abs(_np(Tx)).astype(np.float64) ** 2, RC.true_bins(f_true, freqs_out))


_NP_SHARES = {}


def np_shares(name):
    """{(n_iter, interp): share} of a signal of `SIGNALS` from the restatement in NumPy float64, through the library's
    own design at fs = 1, 32 voices, 'log-piecewise': `reassign_cwt.np_cwt` for the planes, `phase_cwt`'s formula for
    `w`, `statement` for the iteration, the library's bin map (`conceft_cwt.bins`) and a float64 `np.add.at`. Computed
    once per signal."""
    if name in _NP_SHARES:
        return _NP_SHARES[name]
    import reassign_cwt as RC
    import conceft_cwt as C
    from ssqueezepy_amd.padding import pad_geometry
    from ssqueezepy_amd.wavelets import row_frequencies
    kind, N, wavelet = SIGNALS[name]
    x, f = signal(kind, N)
    wav, sc, freqs, const, _ = RC.design(wavelet, N)
    M, n1, _ = pad_geometry(N)
    W, dW = RC.np_cwt(x, wav.fn, sc, M, n1), RC.np_cwt(x, wav.fn, sc, M, n1, deriv=True)
    gamma = 10 * EPS['float64']
    with np.errstate(all='ignore'):
        w = np.abs(np.imag(dW / W)) / (2 * np.pi)
    w[np.abs(W) < gamma] = np.inf
    fr = row_frequencies(wav, sc)
    gk, gp = RC.grid_params(freqs)
    rows = len(sc)
    out = {}
    for n_iter, interp in PASSES:
        wf = statement(w[None], fr, n_iter, interp == 'linear')[0]
        ok = np.isfinite(wf)
        k = C.bins(np.where(ok, wf, 1.), gk, gp, rows - 1)[0]
        k = rows - 1 - k                                                   # flipud
        T = np.zeros(W.shape, dtype=np.complex128)
        cols = np.broadcast_to(np.arange(N)[None, :], W.shape)
        np.add.at(T, (k[ok], cols[ok]), (W * const[:, None])[ok])
        out[(n_iter, interp)] = share(T, f, freqs[::-1])
    _NP_SHARES[name] = out
    return out
