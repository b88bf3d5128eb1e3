# -*- coding: utf-8 -*-
"""What the tests of `ssq_time_reassign` share (tests/test_gpu_tssq_stft.py, its emulated twin and
tests/test_tssq_design.py): the NumPy statement of the entry (include/ssq_hip.h), the
shapes, the seeded planes, the comparison of a device result with the statement, and a NumPy float64 restatement
of the whole transform.

The statement works on separate real float64 arrays with one ufunc per operation, in the stated order: NumPy's
complex multiply may fuse a product into a sum, real ufuncs cannot. The scatter is a Python loop over `c`
(`np.add.at` is not order-safe across versions); the rows and signals of a column are independent -- within one
step no index repeats -- and go through the ufuncs together.
"""
import numpy as np

FS = 200.
EPS = {'float32': float(np.finfo(np.float32).eps), 'float64': float(np.finfo(np.float64).eps)}


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def shapes(seg, max_dmax, s_rows=3):
    """(B, rows, n, n_fft, hop, dmax); `seg`: the segment length the library exports, `max_dmax` the entry's limit,
    `s_rows` the rows of the segment-sized cases."""
    return [(1, 2, 1, 4, 1, 2),                   # smallest case: one column
            (2, 5, 63, 8, 1, 4),                  # less than a block of 64 sources, a second signal
            (1, 3, 64, 16, 4, 2),                 # exactly one block
            (1, 3, 65, 16, 4, 2),                 # a block and one source
            (1, s_rows, seg - 1, 64, 1, 32),      # around one segment
            (1, s_rows, seg, 64, 1, 32),
            (1, s_rows, seg + 1, 64, 1, 32),
            (1, 2, 2 * seg + 7, 256, 1, 128),     # three segments, the halo across both boundaries
            (1, 3, 65, 16, 1, 0),                 # dmax = 0: nothing moves
            (1, 2, 130, 16, 1, max_dmax),         # dmax at the entry's limit
            (2, 5, 63, 8, 1, 200),                # dmax larger than n
            (3, 9, 130, 32, 8, 2)]                # batch


def shape_id(s):
    return 'x'.join(map(str, s))


def rotation_index(i, c, hop, n_fft):
    """``(i c hop) mod n_fft`` for int64 arrays `i` < n_fft and `c`, exact for n_fft < 2^31: every intermediate
    product stays below 2^62."""
    i, c = np.asarray(i, dtype=np.int64), np.asarray(c, dtype=np.int64)
    a = (i * (int(hop) % int(n_fft))) % n_fft
    return (a * (c % n_fft)) % n_fft


def default_rot(n_fft):
    return np.exp(-2j * np.pi * np.arange(n_fft) / n_fft)


def planes(shape, dtype, seed=0):
    """Seeded `Sx` (standard normal), ``Vtg = Sx z`` with `z` standard normal complex scaled so that the displacement
    ``Re(z) cols_per_second`` spans about +-1.5 dmax (two standard deviations): every skip branch is taken."""
    B, rows, n, n_fft, hop, dmax = shape
    rng = np.random.default_rng([seed, B, rows, n, n_fft, hop, min(dmax, 1 << 30)])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    Sx = (rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))).astype(cdt)
    z = rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))
    scale = .75 * max(min(dmax, 4 * n), 1) / (FS / hop)
    return Sx, (Sx * (z * scale)).astype(cdt)


def lower_quartile_gamma(Sx):
    """Midway between two neighbouring samples of ``|Sx|`` at the lower quartile."""
    v = np.sort(np.hypot(Sx.real.astype(np.float64), Sx.imag.astype(np.float64)).reshape(-1))
    k = min(len(v) // 4, len(v) - 2)
    return .5 * (v[k] + v[k + 1])


def near_gamma(Sx, gamma):
    """(B, rows, n): the points with ``| |Sx| - gamma | <= 1e-6 gamma`` -- the device's `hypot` and libm's may put
    such a point on different sides."""
    return np.abs(np.hypot(Sx.real.astype(np.float64), Sx.imag.astype(np.float64)) - gamma) <= 1e-6 * gamma


def terms(Sx, Vtg, rot, n_fft, hop, cps, dmax, gamma):
    """Per point: `ok` (the point is kept and lands on a column), its target column `c2` and its term (vr, vi)."""
    B, rows, n = Sx.shape
    gr, gi = Sx.real.astype(np.float64), Sx.imag.astype(np.float64)
    tr, ti = Vtg.real.astype(np.float64), Vtg.imag.astype(np.float64)
    keep = ~(np.hypot(gr, gi) < gamma)
    with np.errstate(all='ignore'):
        s = np.divide(np.add(np.multiply(tr, gr), np.multiply(ti, gi)),
                      np.add(np.multiply(gr, gr), np.multiply(gi, gi)))
        d = np.rint(np.multiply(s, float(cps)))
        ok = keep & (np.abs(d) <= float(dmax))                  # (false for NaN)
    c2 = np.arange(n, dtype=np.int64) + np.where(ok, d, 0.).astype(np.int64)
    ok &= (c2 >= 0) & (c2 < n)
    if rot is None:
        ur, ui = np.ones((rows, n)), np.zeros((rows, n))
    else:
        p = rotation_index(np.arange(rows)[:, None], np.arange(n)[None, :], hop, n_fft)
        rot = np.asarray(rot, dtype=np.complex128)
        ur, ui = rot.real[p], rot.imag[p]
    with np.errstate(all='ignore'):
        vr = np.subtract(np.multiply(ur, gr), np.multiply(ui, gi))
        vi = np.add(np.multiply(ur, gi), np.multiply(ui, gr))
    return ok, c2, vr, vi


def statement(Sx, Vtg, rot, n_fft, hop, cps, dmax, gamma, reverse=False):
    """`Tx` (B, rows, n) complex128, not yet rounded to an output dtype. `reverse`: the terms in descending `c`
    (what the order tests must be able to tell from the statement)."""
    B, rows, n = Sx.shape
    ok, c2, vr, vi = terms(Sx, Vtg, rot, n_fft, hop, cps, dmax, gamma)
    Tr, Ti = np.zeros((B, rows, n)), np.zeros((B, rows, n))
    for c in (range(n - 1, -1, -1) if reverse else range(n)):
        bb, ii = np.nonzero(ok[:, :, c])                        # one point per (signal, row): no index repeats
        Tr[bb, ii, c2[bb, ii, c]] += vr[bb, ii, c]
        Ti[bb, ii, c2[bb, ii, c]] += vi[bb, ii, c]
    return Tr + 1j * Ti


def check(name, Tx_dev, ref, near):
    """The device's `Tx` against the statement rounded once to its dtype: equal, on every row without a point near
    `gamma`. Returns the number of rows left out."""
    Tx_dev = _np(Tx_dev)
    assert Tx_dev.shape == ref.shape, (name, Tx_dev.shape, ref.shape)
    rows_out = near.any(axis=-1)
    keep = ~rows_out
    want = ref.astype(Tx_dev.dtype)
    assert not np.isnan(Tx_dev).any(), name
    bad = Tx_dev[keep] != want[keep]
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return int(rows_out.sum())


# ------------------------------------------------------------------------------------------ order and conflicts
def to_targets(Sx, target, hop=1):
    """``Vtg`` that sends source `c` of every row to column ``target[c]``: ``Sx (target - c) / cols_per_second``."""
    c = np.arange(Sx.shape[-1])
    return (Sx * ((np.asarray(target) - c) / (FS / hop))).astype(Sx.dtype)


def wide_range_plane(B, rows, n, dtype, seed, target):
    """Standard-normal points; in every cell that receives four sources or more, half of them are replaced by pairs
    ``+v, -v`` with ``|v|`` about 2^20 .. 2^45. The pairs cancel, but on the way the running sum loses the small
    terms' low bits -- which ones depends on the order of the additions, and at a size (2^-12 or so of the result)
    that survives the rounding to float32."""
    rng = np.random.default_rng([seed, B, rows, n])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    P = (rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))).astype(cdt)
    target = np.asarray(target)
    for b in range(B):
        for i in range(rows):
            for cell in np.unique(target):
                src = rng.permutation(np.nonzero(target == cell)[0])
                for k in range(len(src) // 4):
                    v = cdt((rng.standard_normal() + 1j * rng.standard_normal()) * np.exp2(rng.integers(20, 46)))
                    P[b, i, src[2 * k]], P[b, i, src[2 * k + 1]] = v, -v
    return P


def conflict_cases(seg):
    """name -> (n, dmax, target): every source `c` of a row goes to ``target[c]``."""
    n1 = 150
    one = np.full(n1, 70)                                        # every source of a row meets in one cell
    two = np.where(np.arange(n1) % 2 == 0, 60, 85)               # alternate lanes, two cells
    n3 = seg + 200
    c = np.arange(n3)
    # a run that straddles a block of 64 and the segment boundary: [seg-100, seg-20) -> cell seg (the next segment's
    # first), [seg-20, seg+50) -> cell seg-1 (this segment's last); everything else stays
    run = np.where((c >= seg - 100) & (c < seg - 20), seg, np.where((c >= seg - 20) & (c < seg + 50), seg - 1, c))
    return {'one_cell': (n1, 128, one), 'two_cells': (n1, 128, two), 'straddle': (n3, 130, run)}


# ------------------------------------------------------------------------------------------ the whole transform
def gauss_window(n_fft):
    m = np.arange(n_fft) - n_fft // 2
    return np.exp(-.5 * (m / (n_fft / 12.)) ** 2)


def np_stft(x, g, hop):
    """The package's modulated STFT in NumPy float64: reflect extension to ``N + n_fft - 1``, frames of `n_fft`
    every `hop`, window, rotation of the frame centre to index 0, real FFT. (rows, n_hops)."""
    from ssqueezepy_amd.padding import padsignal
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n_fft = len(g)
    xp = padsignal(x, 'reflect', len(x) + n_fft - 1)
    n_hops = (len(xp) - n_fft) // hop + 1
    frames = xp[np.arange(n_fft)[:, None] + hop * np.arange(n_hops)[None, :]] * g[:, None]
    return np.fft.rfft(np.fft.ifftshift(frames, axes=0), axis=0)


def np_tssq(x, g, hop, fs=1., gamma=0.):
    """`tssq_stft` restated in NumPy float64: ``(Tx, Sx)``, each (rows, n_hops)."""
    g = np.asarray(g, dtype=np.float64)
    n_fft = len(g)
    tau = (np.arange(n_fft) - n_fft // 2) / fs
    Sx, Vtg = np_stft(x, g, hop), np_stft(x, tau * g, hop)
    dmax = -(-(n_fft // 2) // hop)
    Tx = statement(Sx[None], Vtg[None], default_rot(n_fft), n_fft, hop, fs / hop, dmax, gamma)[0]
    return Tx, Sx


def dispersive_pulse(N=1024):
    """A pulse whose group delay is ``300 + 100 f`` samples (`f` in cycles/sample) with a Gaussian spectrum centred
    at 0.25, width 0.1."""
    f = np.fft.rfftfreq(N)
    X = np.exp(-.5 * ((f - .25) / .1) ** 2) * np.exp(-2j * np.pi * (300. * f + 50. * f * f))
    return np.fft.irfft(X, N)


def delay_share(P, n_fft, hop):
    """The share of ``|P|^2``, over the rows 0.15 < f < 0.35, within +-1 column of the true group delay."""
    E = np.abs(_np(P)).astype(np.float64) ** 2
    k = np.arange(E.shape[0])
    f = k / n_fft
    rows = np.nonzero((f > .15) & (f < .35))[0]
    col = np.rint((300. + 100. * f) / hop).astype(int)
    hit = sum(E[i, col[i] - 1:col[i] + 2].sum() for i in rows)
    return float(hit / E[rows].sum())
