# -*- coding: utf-8 -*-
"""What the tests of `ssq_reassign_cwt` share (tests/test_gpu_reassign_cwt.py, its emulated twin and
tests/test_reassign_cwt_design.py): the NumPy statement of the entry (include/ssq_hip.h), the
shapes, the seeded and the crafted planes, and a NumPy float64 restatement of the whole transform.

As in tests/reassign2d.py the statement works on separate real float64 arrays with one ufunc per operation, in the
stated order, and the sum is the entry's own: every term is ``np.ldexp(e cst, sh).astype(np.uint64)`` and the scatter is
`np.add.at` on a uint64 array. `reassign2d.shift`, `energy`, `near_gamma`, `quiet_gamma` and `check` are that
module's; the three grids, their bin map `bins` and `NEAR_BOUNDARY` are tests/conceft_cwt.py's. The log maps go through
``log2(w)``, where the device's `log2` and NumPy's may differ by an ulp: the statement reports the kept points whose
fractional bin position lies within `NEAR_BOUNDARY` of a rounding boundary, next to the points near `gamma`, and every
committed seed is one for which it reports none -- the equality checks leave nothing out.
"""
import numpy as np
import reassign2d as R
import conceft_cwt as C
from reassign2d import _np, TWO_PI, EPS  # noqa: F401

GRIDS = C.GRIDS
MAX_DMAX = 1 << 20


# ------------------------------------------------------------------------------------------ the statement
def cell_terms(dmax, n, freq, time=True):
    """`C`: the most terms a cell can receive -- a bin takes points of every row with the frequency axis on, of its own
    row with it off; ``dmax[i]`` counts as 0 with the time axis off."""
    reach = np.minimum(2 * np.asarray(dmax, dtype=np.int64) * int(bool(time)) + 1, int(n))
    return int(reach.sum()) if freq else int(reach.max())


def grid_params(freqs):
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    from ssqueezepy_amd.scales import infer_scaletype
    # (two values are evenly spaced in any metric: `reassign_cwt_gpu` takes them as a linear grid)
    return ssq_grid_params(freqs, len(freqs) > 2 and infer_scaletype(np.asarray(freqs))[0].startswith('log'))


def terms(W, dW, Wd, cst, rsc, dmax, freqs, gamma, flipud=False):
    """Per point: `lands` (kept and not dropped), its target ``(k2, c2)``, its weighted energy `ew`, `kept`, and `near`
    (kept and within `NEAR_BOUNDARY` of a rounding boundary of the bin map). ``dW=None``: the frequency axis is off;
    ``Wd=None``: the time axis is."""
    B, rows, n = W.shape
    gr, gi = W.real.astype(np.float64), W.imag.astype(np.float64)
    e, kept = R.energy(W, gamma)
    lands = kept.copy()
    k2 = np.broadcast_to(np.arange(rows, dtype=np.int64)[None, :, None], W.shape)
    near = np.zeros(W.shape, dtype=bool)
    d = np.zeros(W.shape)
    with np.errstate(all='ignore'):
        if dW is not None:
            dr, di = dW.real.astype(np.float64), dW.imag.astype(np.float64)
            w = np.abs(np.divide(np.subtract(np.multiply(di, gr), np.multiply(dr, gi)), np.multiply(e, TWO_PI)))
            kind, p = grid_params(freqs)
            k, nb = C.bins(w, kind, p, rows - 1)
            near = nb & kept
            k2 = (rows - 1 - k) if flipud else k
        if Wd is not None:
            tr, ti = Wd.real.astype(np.float64), Wd.imag.astype(np.float64)
            s = np.divide(np.subtract(np.multiply(ti, gr), np.multiply(tr, gi)), e)
            d = np.rint(np.multiply(s, np.asarray(rsc, dtype=np.float64)[None, :, None]))
            lands &= np.abs(d) <= np.asarray(dmax, dtype=np.float64)[None, :, None]      # (false for NaN)
        ew = np.multiply(e, np.broadcast_to(np.asarray(cst, dtype=np.float64).reshape(-1), (rows,))[None, :, None])
    c2 = np.arange(n, dtype=np.int64)[None, None, :] + np.where(lands, d, 0.).astype(np.int64)
    lands &= (c2 >= 0) & (c2 < n)
    return lands, k2, c2, ew, kept, near


def statement(W, dW, Wd, cst, rsc, dmax, freqs, gamma, flipud=False):
    """dict: `acc` (B, rows, n) uint64, `peak` (B,) uint64 (the bits of the largest kept term), `sh` (B,) ints, `Rx`
    (B, rows, n) float64 not yet rounded to an output dtype, `q` (the term of every point, 0 where it does not land),
    `lands`, `k2`, `c2`, and the two counts the equality checks rest on: `near_boundary`, `near_gamma`."""
    B, rows, n = W.shape
    lands, k2, c2, ew, kept, near = terms(W, dW, Wd, cst, rsc, dmax, freqs, gamma, flipud)
    Cn = cell_terms(dmax if Wd is not None else np.zeros(rows, dtype=np.int64), n, dW is not None)
    acc = np.zeros((B, rows, n), dtype=np.uint64)
    peak = np.zeros(B, dtype=np.uint64)
    q = np.zeros((B, rows, n), dtype=np.uint64)
    Rx = np.zeros((B, rows, n))
    shs = []
    for b in range(B):
        emax = np.float64(ew[b][kept[b]].max()) if kept[b].any() else np.float64(0.)
        peak[b] = emax.view(np.uint64)
        sh = R.shift(emax, Cn)
        shs.append(sh)
        q[b][lands[b]] = np.ldexp(ew[b][lands[b]], sh).astype(np.uint64)
        np.add.at(acc[b].reshape(-1), (k2[b] * n + c2[b])[lands[b]], q[b][lands[b]])
        Rx[b] = np.ldexp(acc[b].astype(np.float64), -sh)
    return dict(acc=acc, peak=peak, sh=shs, Rx=Rx, q=q, lands=lands, k2=k2, c2=c2, C=Cn,
                near_boundary=int(near.sum()), near_gamma=int(R.near_gamma(W, gamma).sum()))


check = R.check


# ------------------------------------------------------------------------------------------ shapes and planes
def shapes(tr, tc, hr, hc, gcap, wr, wc):
    """(B, rows, n, top): `tr` x `tc` the tile of sources, `hr`, `hc` the window's halo, `wr` x `wc` the window, `gcap` the
    most workgroups of the windowed scatter, as the library exports them; `top` the largest ``dmax[i]``."""
    return [(1, 2, 1, 0),                         # the fewest rows, one column
            (1, 2, 5, 4),                         # the largest dmax a small n allows
            (1, tr - 1, tc - 1, 3),               # around the tile
            (1, tr, tc, 5),
            (1, tr + 1, tc + 1, 7),
            (1, 5, wc - 1, hc - 1),               # around the window's width, the largest dmax around the column halo
            (1, wr, wc, hc),
            (1, wr + 1, wc + 1, hc + 1),
            (2, 5, 63, 200),                      # dmax larger than n
            (3, 9, tc + 40, hc),                  # batch
            (1, 5 * tr, wc + tc, 4 * hc),         # scattered homes: most terms leave the window
            (2, 2, (gcap // 2 + 3) * tc - 5, hc + 1),               # gcap + 6 tiles: some workgroups walk two
            (1, 300, 600, 100)]                   # the workload's row count


SHAPE_IDS = ['one_column', 'small_n_largest_dmax', 'tile_minus_1', 'tile', 'tile_plus_1', 'window_minus_1', 'window',
             'window_plus_1', 'dmax_over_n', 'batch', 'scattered', 'more_tiles_than_workgroups', 'workload_rows']
# The seed of a shape's planes, 0 unless listed: the smallest with which the statement reports no point near a rounding
# boundary of the bin map and none near `gamma`, on every grid, in both dtypes (tests/test_reassign_cwt_design.py asserts
# it for every shape). Seed 0 serves every shape of the list above.
SEEDS = {}


def row_dmax(rows, top):
    """`dmax` (rows,) int32: rising geometrically from 1 to `top` (all 0 for ``top = 0``), the first row's 0 where there
    are more than two rows -- a row whose time axis is off in effect."""
    if top == 0:
        return np.zeros(rows, dtype=np.int32)
    dm = np.rint(np.geomspace(1., float(top), rows)).astype(np.int32)
    if rows > 2:
        dm[0] = 0
    return dm


def planes(shape, dtype, seed=None):
    """Seeded ``(W, dW, Wd, cst, rsc, dmax)``. `W` is standard normal, signal `b` of a batch scaled by ``10^(3 b)`` (so
    that `sh` differs per signal); `dW` is an independent plane scaled as `conceft_cwt.planes` scales it -- the median of
    ``w = |Im(dW / W)| / 2pi`` is about `conceft_cwt.W_MID`, so `w` spans the grids and leaves them at both ends;
    ``Wd = W z`` with the displacements ``Im(z) rsc[i]`` spanning about 1.5 ``dmax[i]`` (two standard deviations): every
    drop branch is taken. `dmax` is `row_dmax`, `rsc` proportional to it, `cst` uniform in [0.5, 2]."""
    B, rows, n, top = shape
    seed = SEEDS.get(tuple(shape), 0) if seed is None else seed
    rng = np.random.default_rng([seed, B, rows, n, top, 1995])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    amp = (10. ** (3 * np.arange(B)))[:, None, None]
    W = ((rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))) * amp).astype(cdt)
    dW = ((rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))) * amp
          * (C.W_MID * TWO_PI * np.sqrt(3.))).astype(cdt)
    dmax = row_dmax(rows, top)
    rsc = 3. * np.maximum(dmax, .5)
    z = rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))
    Wd = (W * (z * (.75 * dmax / rsc)[None, :, None])).astype(cdt)
    cst = rng.uniform(.5, 2., rows)
    return W, dW, Wd, cst, rsc, dmax


def crafted(amp, k, d, freqs, rsc, dtype):
    """Planes that give chosen targets exactly: ``W = amp`` (real), ``dW = 2 pi i f W`` with ``f = freqs[k]`` a bin's own
    frequency (`k` may also be given as frequencies through a float array), ``Wd = i (d / rsc[i]) W``; `amp`, `k`, `d`
    broadcast to one (B, rows, n) shape. The quotients come back to within a few ulp of the data type: `w` at a bin's
    centre, far from a rounding boundary, and ``Im(Wd / W) rsc[i]`` within 1e-5 of the integer `d`."""
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    freqs = np.asarray(freqs, dtype=np.float64)
    k = np.asarray(k)
    f = freqs[k] if k.dtype.kind in 'iu' else k.astype(np.float64)
    amp, f, d = np.broadcast_arrays(np.asarray(amp, dtype=np.float64), f, np.asarray(d, dtype=np.float64))
    W = amp.astype(cdt)
    dW = (W.astype(np.complex128) * (1j * TWO_PI * f)).astype(cdt)
    Wd = (W.astype(np.complex128) * (1j * d / np.asarray(rsc, dtype=np.float64)[None, :, None])).astype(cdt)
    return W, dW, Wd


# ------------------------------------------------------------------------------------------ the whole transform
def np_cwt(x, fn, scales, M, n1, deriv=False):
    """``ifft(fn(a xi) fft(pad x))`` (times ``1j xi`` for the time derivative, fs = 1) in float64: reflect padding to
    `M`, the Nyquist bin halved, as the plans do it."""
    N = len(x)
    xp = np.pad(np.asarray(x, dtype=np.float64), (n1, M - N - n1), mode='reflect')
    k = np.arange(M)
    xi = np.where(k <= M // 2, k, k - M) * (2 * np.pi / M)
    with np.errstate(all='ignore'):
        P = np.asarray(fn(np.asarray(scales, dtype=np.float64).reshape(-1, 1) * xi)).astype(np.float64)
    P[:, M // 2] /= 2
    xh = np.fft.fft(xp)
    if deriv:
        xh = xh * (1j * xi)
    return np.fft.ifft(P * xh, axis=-1)[:, n1:n1 + N]


def design(wavelet, N, scales='log-piecewise', nv=32):
    """``(wav64, scales, ssq_freqs, const, dmax)`` of `reassign_cwt`'s defaults at fs = 1, the wavelet in float64."""
    from ssqueezepy_amd import Wavelet, algos, wavelet_time_std
    from ssqueezepy_amd._cwt import _process_gmw_wavelet
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    wav = Wavelet(_process_gmw_wavelet(wavelet, True), N=N, dtype='float64')
    sc, freqs, const, _, _ = _ssq_design(wav, scales, nv, N, 1., None, 'peak', True)
    sc = np.asarray(sc, dtype=np.float64).reshape(-1)
    const = np.broadcast_to(np.asarray(const, dtype=np.float64).reshape(-1), sc.shape)
    return wav, sc, np.asarray(freqs, dtype=np.float64), const, algos.reassign_cwt_dmax(sc, wavelet_time_std(wav), 4.)


def np_planes(x, wav, sc):
    """``(W, dW, Wd)`` of a 1-D signal in NumPy float64."""
    from ssqueezepy_amd.padding import pad_geometry
    from ssqueezepy_amd.wavelets import derived_wavelets
    M, n1, _ = pad_geometry(len(x))
    psih = wav.fn
    dpsih = derived_wavelets(wav)[0].fn
    return np_cwt(x, psih, sc, M, n1), np_cwt(x, psih, sc, M, n1, deriv=True), np_cwt(x, dpsih, sc, M, n1)


def np_reassign(W, dW, Wd, sc, freqs, const, dmax, gamma, mode='both', flipud=True):
    """The energy plane of `reassign_cwt` from NumPy planes: `terms`, then a float64 `np.add.at` of ``|W|^2 const[i]``
    (no fixed point: the restatement is of the transform, not of the sum)."""
    lands, k2, c2, ew, _, _ = terms(W[None], dW[None] if mode != 'time' else None, Wd[None] if mode != 'freq' else None,
                                    const, sc, dmax, freqs, gamma, flipud)
    n = W.shape[-1]
    A = np.zeros(W.shape)
    np.add.at(A.reshape(-1), (k2[0] * n + c2[0])[lands[0]], ew[0][lands[0]])
    return A


def fm_tone(N=4096, period=300.):
    """``cos`` of the phase whose frequency is ``0.15 + 0.05 cos(2 pi t / period)`` cycles per sample; returns (x, f)."""
    t = np.arange(N)
    f = .15 + .05 * np.cos(2 * np.pi * t / period)
    return np.cos(2 * np.pi * np.cumsum(f)), f


def true_bins(f, freqs_out):
    """The row of `freqs_out` (the order the transform returns: high to low with `flipud`) nearest to every `f`, in
    log-frequency."""
    return np.abs(np.log(np.asarray(freqs_out, dtype=np.float64))[:, None] - np.log(f)[None, :]).argmin(axis=0)


def row_freqs(wav, sc):
    """The rows' own centre frequencies, cycles per sample: the wavelet's continuous-time peak over the scale. They are
    what a row of the scalogram, and of ``reassign='time'`` (which keeps a point in its row), stands for; `ssq_freqs` is
    what a bin stands for, and the two differ -- the grid's top is clipped at Nyquist, four bins below the first row's
    centre for a Morlet wavelet of mu = 13.4."""
    from ssqueezepy_amd.wavelets import center_frequency
    return center_frequency(wav, kind='peak-ct') / (2 * np.pi * np.asarray(sc, dtype=np.float64))


def fm_shares(planes, f, freqs_out, rows_out):
    """The four shares from the four planes ``(scalogram, 'freq', 'time', 'both')``: the bin-indexed ones against the true
    bin on `freqs_out`, the row-indexed ones against the true row on `rows_out`."""
    kbin, krow = true_bins(f, freqs_out), true_bins(f, rows_out)
    return [ridge_share(E, k) for E, k in zip(planes, (krow, kbin, krow, kbin))]


def ridge_share(E, kbin):
    """`reassign2d.ridge_share` on a bin grid: the share of `E` (rows, n), over the interior three quarters of the
    columns, within +-1 row of the true bin ``kbin[c]``."""
    E = np.abs(_np(E)).astype(np.float64)
    rows, n = E.shape
    cols = np.arange(n // 8, n - n // 8)
    k = kbin[cols]
    hit = sum(E[np.clip(k + o, 0, rows - 1), cols][(k + o >= 0) & (k + o < rows)].sum() for o in (-1, 0, 1))
    return float(hit / E[:, cols].sum())


_SHARES = {}


def np_fm_shares(period=300., N=4096, mu=13.4, nv=32):
    """The four shares of the FM tone -- scalogram, 'freq', 'time', 'both' -- from the restatement, through the library's
    own design (``('morlet', mu)``, `nv` voices, 'log-piecewise'); computed once per argument set."""
    key = (period, N, mu, nv)
    if key not in _SHARES:
        x, f = fm_tone(N, period)
        wav, sc, freqs, const, dmax = design(('morlet', {'mu': mu}), N, nv=nv)
        W, dW, Wd = np_planes(x, wav, sc)
        gamma = 10 * EPS['float64']
        planes = [np.abs(W) ** 2 * const[:, None]]
        planes += [np_reassign(W, dW, Wd, sc, freqs, const, dmax, gamma, mode) for mode in ('freq', 'time', 'both')]
        _SHARES[key] = fm_shares(planes, f, freqs[::-1], row_freqs(wav, sc))
    return _SHARES[key]
