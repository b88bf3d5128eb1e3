# -*- coding: utf-8 -*-
"""What the tests of `ssq_multi_squeeze` share (tests/test_gpu_msst_stft.py, its emulated twin and
tests/test_msst_design.py): the NumPy statement of the iteration (include/ssq_hip.h), the
launcher's sizing restated, the seeded and the order planes, the signals and the +-1-bin share metric.

The statement works on separate float64 arrays with one ufunc per operation and a Python loop over the iterations; all
points of all columns go through the ufuncs together (a point reads `w`, which nobody writes). It returns `w_final`
rounded to the dtype. The expected `Tx` is then `indexed_sum_onfly(Sx, w_final, ...)`: that entry is pinned to the
oracle and ordered, so it states the binning and the accumulation, summation order included.
"""
import numpy as np

EPS = {'float32': float(np.finfo(np.float32).eps), 'float64': float(np.finfo(np.float64).eps)}
LDS_BYTES = 160 * 1024          # per CU on gfx950
TILE_COLS = (16, 8, 4)          # the launcher's tile widths, widest first
REALS_PER_ROW = 3               # LDS per row and column: a complex Tx cell and a w


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def tile_rows(dtype, cols):
    """The most rows a tile of `cols` columns holds: the launcher takes the widest tile that fits, so one row more
    takes the next narrower one, and `tile_rows(dtype, 4)` is `ssq_multi_squeeze_max_rows`."""
    return LDS_BYTES // (cols * REALS_PER_ROW * np.dtype(dtype).itemsize)


def row_grid(Sfs):
    """(f0, df) as `multi_squeeze_gpu` takes them from `Sfs`: float64 of the first value and of the first step."""
    v = np.asarray(Sfs).astype(np.float64)
    return float(v[0]), float(v[1] - v[0])


def statement(w, f0, df, n_iter, interp):
    """`w_final` of the dtype of `w` (B, rows, n): the entry's iteration, ``inf`` where ``w`` is not finite."""
    W = np.asarray(w).astype(np.float64)
    rows = W.shape[1]
    have = np.isfinite(W)
    f, moving = W.copy(), have.copy()
    with np.errstate(all='ignore'):
        for _ in range(int(n_iter) - 1):
            if not moving.any():
                break
            p = np.divide(np.subtract(f, f0), df)
            inside = moving & (p >= 0.) & (p <= float(rows - 1))          # (false for NaN)
            ps = np.where(inside, p, 0.)
            g = np.take_along_axis(W, np.rint(ps).astype(np.int64), axis=1)
            if interp:
                i0 = np.minimum(np.floor(ps).astype(np.int64), rows - 2)
                a = np.subtract(ps, i0.astype(np.float64))
                wa, wc = np.take_along_axis(W, i0, axis=1), np.take_along_axis(W, i0 + 1, axis=1)
                lerp = np.add(wa, np.multiply(a, np.subtract(wc, wa)))
                g = np.where(np.isfinite(wa) & np.isfinite(wc), lerp, g)
            ok = inside & np.isfinite(g)
            moving = ok & (g != f)
            f = np.where(ok, g, f)
    return np.where(have, f, np.inf).astype(np.asarray(w).dtype)


def make_Sfs(rows, dtype, fs=200.):
    return np.linspace(0, .5 * fs, rows).astype(dtype)


def planes(B, rows, n, dtype, seed=0):
    """Seeded `Sx` (standard normal), `w` uniform over 1.5 times the rows' range (a quarter below, a quarter above:
    some points leave the grid), a quarter of the points ``inf``; `Sfs`."""
    rng = np.random.default_rng([seed, B, rows, n])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    Sx = (rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))).astype(cdt)
    Sfs = make_Sfs(rows, dtype)
    span = float(Sfs[-1] - Sfs[0])
    w = (Sfs[0] + span * rng.uniform(-.25, 1.25, (B, rows, n))).astype(dtype)
    w[rng.uniform(size=w.shape) < .25] = np.inf
    return Sx, w, Sfs


# ------------------------------------------------------------------------------------------ order
def order_planes(dtype, rows=40, n=5, seed=5):
    """name -> (Sx, w, Sfs, n_iter, the row every row ends on): every row of a column walks two rows per pass towards the target of its parity
    -- one target (`one_bin`: rows 20 and 21 hold `Sfs[20]`) or two (`two_bins`: 10 for even rows, 31 for odd ones) --
    on a grid whose arithmetic is exact (``Sfs = 2 + i / 2``). `Sx`: the cancelling-pair planes of the tssq tests,
    pairs up to 2^45 among terms of order 1, per column along the rows."""
    import tssq
    Sfs = (2. + .5 * np.arange(rows)).astype(dtype)
    i = np.arange(rows)
    out = {}
    for name, (t_even, t_odd) in {'one_bin': (20, 21), 'two_bins': (10, 31)}.items():
        tq = np.where(i % 2 == 0, t_even, t_odd)
        nxt = i + 2 * np.sign(tq - i)
        final = np.where(i % 2 == 0, t_even, t_odd if name == 'two_bins' else t_even)
        wcol = Sfs[nxt].copy()
        if name == 'one_bin':
            wcol[t_odd] = Sfs[t_even]
        P = tssq.wide_range_plane(1, n, rows, dtype, seed, final)              # (1, n, rows): pairs per target cell
        Sx = np.ascontiguousarray(np.swapaxes(P, 1, 2))
        w = np.ascontiguousarray(np.broadcast_to(wcol[None, :, None], (1, rows, n))).astype(dtype)
        out[name] = (Sx, w, Sfs, rows, final)
    return out


def ordered_sum(Sx, bins, const, reverse=False):
    """``Tx[k] += Sx[i] * const`` in ascending (descending: `reverse`) `i`, in the dtype of `Sx`, on (1, rows, n)
    planes with one bin per row."""
    Tx = np.zeros_like(Sx)
    rdt = Sx.real.dtype.type
    rows = Sx.shape[1]
    for i in (range(rows - 1, -1, -1) if reverse else range(rows)):
        Tx[:, bins[i], :] += (Sx[:, i, :].real * rdt(const) + 1j * (Sx[:, i, :].imag * rdt(const))).astype(Sx.dtype)
    return Tx


# ------------------------------------------------------------------------------------------ signals and the metric
FS = 1024.
N_FFT = 256


def gauss_window(n_fft=N_FFT):
    """Gaussian, sigma = n_fft / 8 samples."""
    m = np.arange(n_fft) - n_fft // 2
    return np.exp(-.5 * (m / (n_fft / 8.)) ** 2)


def signal(name, N=1024, fs=FS):
    """(x, instantaneous frequency in Hz): the issue's linear chirp 50 -> 450 Hz, quadratic chirp 50 -> 450 Hz and FM
    tone 150 +- 60 Hz at 2 Hz, over `N` samples at `fs`."""
    t = np.arange(N) / fs
    T = N / fs
    if name == 'linear':
        f = 50. + 400. * t / T
        ph = 50. * t + 200. * t * t / T
    elif name == 'quadratic':
        f = 50. + 400. * (t / T) ** 2
        ph = 50. * t + 400. * t ** 3 / (3. * T * T)
    else:
        f = 150. + 60. * np.cos(2 * np.pi * 2. * t)
        ph = 150. * t + 60. / (2 * np.pi * 2.) * np.sin(2 * np.pi * 2. * t)
    return np.cos(2 * np.pi * ph), f


def share(Tx, f_true, ssq_freqs, n_fft=N_FFT):
    """The share of ``|Tx|^2``, over the columns [n_fft, N - n_fft), within +-1 bin of the true frequency."""
    E = np.abs(_np(Tx)).astype(np.float64) ** 2
    v = np.asarray(ssq_freqs, dtype=np.float64)
    N = E.shape[-1]
    cols = np.arange(n_fft, N - n_fft)
    k = np.rint((f_true[cols] - v[0]) / (v[1] - v[0])).astype(int)
    hit = sum(E[max(kk - 1, 0):kk + 2, c].sum() for kk, c in zip(k, cols))
    return float(hit / E[:, cols].sum())
