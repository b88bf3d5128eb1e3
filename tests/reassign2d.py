# -*- coding: utf-8 -*-
"""What the tests of `ssq_reassign2d` share (tests/test_gpu_reassign_stft.py, its emulated twin and
tests/test_reassign_design.py): the NumPy statement of the entry (include/ssq_hip.h), the
shapes, the seeded and the crafted planes, and the comparison of a device result with the statement.

The statement works on separate real float64 arrays with one ufunc per operation, in the stated order (NumPy's
complex arithmetic may fuse a product into a sum, real ufuncs cannot). The sum is the entry's own: every term is
``np.ldexp(e, sh).astype(np.uint64)`` and the scatter is `np.add.at` on a uint64 array -- integer addition, so the
order `np.add.at` takes is of no concern.
"""
import numpy as np

FS = 200.
TWO_PI = 6.283185307179586
EPS = {'float32': float(np.finfo(np.float32).eps), 'float64': float(np.finfo(np.float64).eps)}


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


# ------------------------------------------------------------------------------------------ the statement
def cell_terms(rows, n, dmax):
    """`C`: the most terms a cell can receive."""
    return int(rows) * min(2 * int(dmax) + 1, int(n))


def shift(emax, C):
    """``sh = 62 - H - ex``: `H` the bit length of `C`, `ex` `frexp(emax)`'s exponent."""
    return 62 - int(C).bit_length() - int(np.frexp(np.float64(emax))[1])


def energy(Sx, gamma):
    """``(e, kept)``: the float64 energy of every point, and whether the point is kept."""
    gr, gi = Sx.real.astype(np.float64), Sx.imag.astype(np.float64)
    with np.errstate(all='ignore'):
        e = np.add(np.multiply(gr, gr), np.multiply(gi, gi))
        mag = np.sqrt(e) if Sx.dtype == np.complex64 else np.hypot(gr, gi)
        kept = ~(mag < gamma) & np.isfinite(e)
    return e, kept


def near_gamma(Sx, gamma):
    """The points with ``| |Sx| - gamma | <= 1e-6 gamma``: the device's `hypot` and libm's may put such a point on
    different sides."""
    return np.abs(np.hypot(Sx.real.astype(np.float64), Sx.imag.astype(np.float64)) - gamma) <= 1e-6 * gamma


def terms(Sx, dSx, Vtg, n_fft, fs, cps, kmax, dmax, gamma):
    """Per point: `lands` (kept and not dropped), its target ``(k2, c2)``, its energy `e` and `kept`. ``dSx=None``:
    the frequency axis is off; ``Vtg=None`` or ``dmax=0``: the time axis is."""
    B, rows, n = Sx.shape
    gr, gi = Sx.real.astype(np.float64), Sx.imag.astype(np.float64)
    e, kept = energy(Sx, gamma)
    lands = kept.copy()
    m, d = np.zeros(Sx.shape), np.zeros(Sx.shape)
    with np.errstate(all='ignore'):
        if dSx is not None:
            dr, di = dSx.real.astype(np.float64), dSx.imag.astype(np.float64)
            im = np.divide(np.subtract(np.multiply(di, gr), np.multiply(dr, gi)), e)
            m = np.rint(np.divide(np.divide(np.negative(im), TWO_PI), np.divide(float(fs), float(n_fft))))
            lands &= np.abs(m) <= float(kmax)                       # (false for NaN)
        if Vtg is not None and dmax != 0:
            tr, ti = Vtg.real.astype(np.float64), Vtg.imag.astype(np.float64)
            s = np.divide(np.add(np.multiply(tr, gr), np.multiply(ti, gi)), e)
            d = np.rint(np.multiply(s, float(cps)))
            lands &= np.abs(d) <= float(dmax)
    k2 = np.abs(np.arange(rows, dtype=np.int64)[None, :, None] + np.where(lands, m, 0.).astype(np.int64))
    c2 = np.arange(n, dtype=np.int64)[None, None, :] + np.where(lands, d, 0.).astype(np.int64)
    lands &= (k2 <= rows - 1) & (c2 >= 0) & (c2 < n)
    return lands, k2, c2, e, kept


def statement(Sx, dSx, Vtg, n_fft, fs, cps, kmax, dmax, gamma):
    """dict: `acc` (B, rows, n) uint64, `peak` (B,) uint64 (the bits of the largest kept energy), `sh` (B,) ints, `Rx`
    (B, rows, n) float64 not yet rounded to an output dtype, `q` (the term of every point, 0 where it does not land),
    `lands`, `k2`, `c2`."""
    B, rows, n = Sx.shape
    lands, k2, c2, e, kept = terms(Sx, dSx, Vtg, n_fft, fs, cps, kmax, dmax, gamma)
    C = cell_terms(rows, n, dmax if Vtg is not None else 0)
    acc = np.zeros((B, rows, n), dtype=np.uint64)
    peak = np.zeros(B, dtype=np.uint64)
    q = np.zeros((B, rows, n), dtype=np.uint64)
    Rx = np.zeros((B, rows, n))
    shs = []
    for b in range(B):
        emax = np.float64(e[b][kept[b]].max()) if kept[b].any() else np.float64(0.)
        peak[b] = emax.view(np.uint64)
        sh = shift(emax, C)
        shs.append(sh)
        q[b][lands[b]] = np.ldexp(e[b][lands[b]], sh).astype(np.uint64)
        np.add.at(acc[b].reshape(-1), (k2[b] * n + c2[b])[lands[b]], q[b][lands[b]])
        Rx[b] = np.ldexp(acc[b].astype(np.float64), -sh)
    return dict(acc=acc, peak=peak, sh=shs, Rx=Rx, q=q, lands=lands, k2=k2, c2=c2)


def check(name, got, ref, dtype):
    """``(Rx, acc, peak)`` of the device against the statement: `acc` and `peak` equal as integers, `Rx` equal to the
    statement's rounded once to `dtype`."""
    Rx, acc, peak = (_np(a) for a in got)
    assert Rx.dtype == np.dtype(dtype), (name, Rx.dtype)
    want_acc, want_peak = ref['acc'].reshape(acc.shape), ref['peak']
    assert np.array_equal(peak.view(np.uint64), want_peak), (name, peak, want_peak)
    bad = acc.view(np.uint64) != want_acc
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert int(want_acc.max()) < 2 ** 62, name
    assert np.array_equal(Rx, ref['Rx'].reshape(Rx.shape).astype(dtype)), name


# ------------------------------------------------------------------------------------------ shapes and planes
def shapes(tr, tc, hr, hc, gcap):
    """(B, rows, n, dmax, kmax, spread): `tr` x `tc` the tile of sources, `hr`, `hc` the window's halo, `gcap` the most
    workgroups of the windowed scatter, as the library exports them; `spread` scales the rows' displacements (in rows,
    two standard deviations)."""
    wc = tc + 2 * hc
    return [(1, 1, 1, 0, 0, 1),                   # one point
            (1, 2, 5, 4, 1, 2),                   # the largest dmax a small n allows
            (1, 63, tc - 1, 1, 1, 2),             # around the tile's width
            (1, 64, tc, hc - 1, 1, 2),            # ... dmax one below the column halo
            (1, 65, tc + 1, hc, 1, 2),            # ... at it
            (1, 129, wc - 1, hc + 1, 1, 2),       # around the window's width; dmax beyond the halo
            (1, 2, wc, 0, 1, 2),                  # dmax = 0: nothing moves along the row
            (1, 3, wc + 1, hc + 1, 0, 2),         # kmax = 0
            (1, tr + 1, 2 * tc + 1, 2 * hc, hr + 1, hr + 1),        # row displacements up to the row halo and past it
            (3, 9, tc + 40, hc, 1, 2),            # batch
            (2, 5, 63, 200, 1, 2),                # dmax larger than n
            (1, 5 * tr, wc + tc, 4 * hc, 5 * tr, 6 * hr + 12),      # scattered: most terms leave the window
            (2, 2, (gcap // 2 + 3) * tc - 5, hc + 1, 1, 2)]         # gcap + 6 tiles: some workgroups walk two


SHAPE_IDS = ['one_point', 'small_n_largest_dmax', 'tile_minus_1', 'tile', 'tile_plus_1', 'window_minus_1',
             'window_dmax_0', 'window_plus_1_kmax_0', 'past_row_halo', 'batch', 'dmax_over_n', 'scattered', 'more_tiles_than_workgroups']


def planes(shape, dtype, seed=0):
    """Seeded `Sx` (standard normal; signal `b` of a batch scaled by ``10^(3 b)``, so that `sh` differs per signal),
    ``dSx = Sx z1`` and ``Vtg = Sx z2`` with the displacements spanning about 1.5 times `kmax`-or-`spread` rows and 1.5
    `dmax` columns (two standard deviations): every drop branch is taken. n_fft = 2 rows."""
    B, rows, n, dmax, kmax, spread = shape
    rng = np.random.default_rng([seed, B, rows, n, min(dmax, 1 << 30), kmax, spread])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    Sx = rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))
    Sx = (Sx * (10. ** (3 * np.arange(B)))[:, None, None]).astype(cdt)
    z1 = rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))
    z2 = rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))
    df = FS / (2 * rows)
    dSx = (Sx * (z1 * (.75 * spread * TWO_PI * df))).astype(cdt)
    Vtg = (Sx * (z2 * (.75 * max(min(dmax, 4 * n), 1) / FS))).astype(cdt)
    return Sx, dSx, Vtg


def lower_quartile_gamma(Sx):
    """Midway between two neighbouring samples of ``|Sx|`` at the lower quartile."""
    v = np.sort(np.hypot(Sx.real.astype(np.float64), Sx.imag.astype(np.float64)).reshape(-1))
    if len(v) < 2:
        return .5 * float(v[0])
    k = min(len(v) // 4, len(v) - 2)
    return .5 * (v[k] + v[k + 1])


def quiet_gamma(Sx):
    """A `gamma` near the lower quartile of the first signal's ``|Sx|``, midway between two neighbouring samples (of
    any signal) that lie more than 3e-6 (relative) apart: no point is within 1e-6 of it, however many points there are."""
    v = np.sort(np.hypot(Sx.real.astype(np.float64), Sx.imag.astype(np.float64)).reshape(-1))
    start = lower_quartile_gamma(Sx[0])
    for k in range(max(int(np.searchsorted(v, start)) - 1, 0), len(v) - 1):
        mid = .5 * (v[k] + v[k + 1])
        if v[k + 1] - v[k] > 3e-6 * mid:
            return mid
    return start


def crafted(amp, m, d, dtype, n_fft, fs=FS, cps=FS):
    """Planes that give integer displacements exactly: ``Sx = amp`` (real), ``dSx = -2 pi i m (fs / n_fft) Sx``,
    ``Vtg = (d / cps) Sx``; `amp`, `m`, `d` broadcast to one (B, rows, n) shape. The quotients come back as `m` and `d`
    to within a few ulp of the data type, far from a tie."""
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    amp, m, d = np.broadcast_arrays(np.asarray(amp, dtype=np.float64), np.asarray(m, dtype=np.float64),
                                    np.asarray(d, dtype=np.float64))
    Sx = amp.astype(cdt)
    dSx = (Sx.astype(np.complex128) * (-1j * TWO_PI * m * (fs / n_fft))).astype(cdt)
    Vtg = (Sx.astype(np.complex128) * (d / cps)).astype(cdt)
    return Sx, dSx, Vtg


# ------------------------------------------------------------------------------------------ the whole transform
def gauss_window(n_fft=256, sigma=24.):
    m = np.arange(n_fft) - n_fft // 2
    return np.exp(-.5 * (m / sigma) ** 2)


def fm_tone(N=4096):
    """``cos`` of the phase whose frequency is ``0.25 + 0.08 cos(2 pi t / 600)`` cycles per sample; returns (x, f)."""
    t = np.arange(N)
    f = .25 + .08 * np.cos(2 * np.pi * t / 600.)
    return np.cos(2 * np.pi * np.cumsum(f)), f


def ridge_share(E, f, n_fft, hop):
    """The share of `E` (rows, n), over the interior three quarters of the columns, within +-1 row of the true
    frequency ``f[c hop]``."""
    E = np.abs(_np(E)).astype(np.float64)
    n = E.shape[-1]
    cols = np.arange(n // 8, n - n // 8)
    k = np.rint(f[cols * hop] * n_fft).astype(int)
    hit = sum(E[k + o, cols].sum() for o in (-1, 0, 1))
    return float(hit / E[:, cols].sum())


def np_shares(hop, weight='energy', N=4096, n_fft=256, sigma=24.):
    """The four shares of the FM tone -- spectrogram, 'freq', 'time', 'both' -- from a NumPy float64 restatement of the
    whole transform: `tssq.np_stft` with the window, its spectral derivative and ``tau`` times it, `terms`, and a float64
    `np.add.at` of ``|Sx|^2`` (`weight` 'amplitude': of ``|Sx|``, which is not the transform)."""
    import tssq
    from ssqueezepy_amd._stft import _spectral_derivative
    x, f = fm_tone(N)
    g = gauss_window(n_fft, sigma)
    tau = np.arange(n_fft) - float(n_fft // 2)
    S = tssq.np_stft(x, g, hop)
    dS = tssq.np_stft(x, np.asarray(_spectral_derivative(g)).real, hop)
    V = tssq.np_stft(x, tau * g, hop)
    w = np.abs(S) ** 2 if weight == 'energy' else np.abs(S)
    n = S.shape[1]
    out = [ridge_share(w, f, n_fft, hop)]
    for fr, ti in ((1, 0), (0, 1), (1, 1)):
        lands, k2, c2, _, _ = terms(S[None], dS[None] if fr else None, V[None] if ti else None, n_fft, 1., 1. / hop,
                                    n_fft // 2, -(-(n_fft // 2) // hop), 1e-12)
        A = np.zeros(S.shape)
        np.add.at(A.reshape(-1), (k2[0] * n + c2[0])[lands[0]], w[lands[0]])
        out.append(ridge_share(A, f, n_fft, hop))
    return out
