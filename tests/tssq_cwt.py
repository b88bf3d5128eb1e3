# -*- coding: utf-8 -*-
"""What the tests of `ssq_time_reassign_cwt` share (tests/test_gpu_tssq_cwt.py, its emulated twin and
tests/test_tssq_cwt_design.py): the NumPy statement of the entry (include/ssq_hip.h), the
shapes, the seeded planes, the host form of the rotation tables, and a NumPy float64 restatement of the whole transform.

As in tests/reassign_cwt.py the statement works on separate real float64 arrays with one ufunc per operation, in the
stated order, and the sum is the entry's own: every component of a term is ``np.trunc(np.ldexp(z, sh)).astype(np.int64)``
and the scatter is `np.add.at` on an int64 array. Every operation is a basic IEEE one but the `hypot` of float64 planes in
the point test, so the statement reports the points within 1e-6 (relative) of `gamma`, and every committed case is one
for which it reports none -- the equality checks leave nothing out.
"""
import numpy as np
import reassign2d as R
import reassign_cwt as RC
from reassign2d import _np, EPS  # noqa: F401

P = 256                 # SSQ_TSSQ_CWT_ROT_P (ssq_time_reassign_cwt_tile(5); the GPU module asserts it)
MAX_DMAX = 1 << 20


# ------------------------------------------------------------------------------------------ the statement
def tables(phi, n):
    """``(rot_lo, rot_hi)`` complex128 on the host, as `algos.cwt_rotation_tables` makes them for ``fs = 1``."""
    from ssqueezepy_amd import algos
    phi = np.asarray(phi, dtype=np.float64).reshape(-1)
    return (np.exp(-2j * np.pi * algos._exact_turns(phi, 1, P)),
            np.exp(-2j * np.pi * algos._exact_turns(phi, P, -(-int(n) // P))))


def cell_terms(dmax, n):
    """`C`: the most terms a cell can receive -- the points of its own row within the row's bound."""
    return int(np.minimum(2 * np.asarray(dmax, dtype=np.int64) + 1, int(n)).max())


def shift(emax, C):
    """``sh = 61 - H - hx``: `H` the bit length of `C`, ``hx = ceil(ex / 2)``, `ex` `frexp(emax)`'s exponent."""
    ex = int(np.frexp(np.float64(emax))[1])
    return 61 - int(C).bit_length() - (-((-ex) // 2))


def terms(W, Wd, rsc, dmax, rot, gamma):
    """Per point: `lands` (kept and not dropped), its target column `c2`, the rotated term ``(zr, zi)``, the energy `e`
    and `kept`. ``rot = None``: no rotation; else the ``(rot_lo, rot_hi)`` pair, host complex128."""
    B, rows, n = W.shape
    gr, gi = W.real.astype(np.float64), W.imag.astype(np.float64)
    e, kept = R.energy(W, gamma)
    with np.errstate(all='ignore'):
        tr, ti = Wd.real.astype(np.float64), Wd.imag.astype(np.float64)
        s = np.divide(np.subtract(np.multiply(ti, gr), np.multiply(tr, gi)), e)
        d = np.rint(np.multiply(s, np.asarray(rsc, dtype=np.float64)[None, :, None]))
        lands = kept & (np.abs(d) <= np.asarray(dmax, dtype=np.float64)[None, :, None])         # (false for NaN)
        c2 = np.arange(n, dtype=np.int64)[None, None, :] + np.where(lands, d, 0.).astype(np.int64)
        lands &= (c2 >= 0) & (c2 < n)
        if rot is None:
            zr, zi = gr, gi
        else:
            lo, hi = rot
            c = np.arange(n)
            lr, li = lo.real[:, c % P][None], lo.imag[:, c % P][None]
            hr, hi_ = hi.real[:, c // P][None], hi.imag[:, c // P][None]
            ur = np.subtract(np.multiply(hr, lr), np.multiply(hi_, li))
            ui = np.add(np.multiply(hr, li), np.multiply(hi_, lr))
            zr = np.subtract(np.multiply(ur, gr), np.multiply(ui, gi))
            zi = np.add(np.multiply(ur, gi), np.multiply(ui, gr))
    return lands, c2, zr, zi, e, kept


def statement(W, Wd, rsc, dmax, rot, gamma):
    """dict: `acc` (B, rows, n, 2) int64, `peak` (B,) uint64 (the bits of the largest kept energy), `sh` (B,) ints, `Tx`
    (B, rows, n) complex128 not yet rounded to an output dtype, `q` (B, rows, n, 2) int64 (the term of every point, 0
    where it does not land), `lands`, `c2`, `C`, and the count the equality checks rest on, `near_gamma`."""
    B, rows, n = W.shape
    lands, c2, zr, zi, e, kept = terms(W, Wd, rsc, dmax, rot, gamma)
    Cn = cell_terms(dmax, n)
    acc = np.zeros((B, rows, n, 2), dtype=np.int64)
    q = np.zeros((B, rows, n, 2), dtype=np.int64)
    peak = np.zeros(B, dtype=np.uint64)
    Tx = np.zeros((B, rows, n), dtype=np.complex128)
    shs = []
    cell = np.arange(rows, dtype=np.int64)[:, None] * n
    for b in range(B):
        emax = np.float64(e[b][kept[b]].max()) if kept[b].any() else np.float64(0.)
        peak[b] = emax.view(np.uint64)
        sh = shift(emax, Cn)
        shs.append(sh)
        L = lands[b]
        for k, z in enumerate((zr, zi)):
            q[b, ..., k][L] = np.trunc(np.ldexp(z[b][L], sh)).astype(np.int64)
            np.add.at(acc[b, ..., k].reshape(-1), (cell + c2[b])[L], q[b, ..., k][L])
        Tx[b] = np.ldexp(acc[b, ..., 0].astype(np.float64), -sh) + 1j * np.ldexp(acc[b, ..., 1].astype(np.float64), -sh)
    return dict(acc=acc, peak=peak, sh=shs, Tx=Tx, q=q, lands=lands, c2=c2, C=Cn,
                near_gamma=int(R.near_gamma(W, gamma).sum()))


def check(name, got, ref, dtype):
    """``(Tx, acc, peak)`` of the device against the statement: `acc` and `peak` equal as integers, `Tx` equal to the
    statement's rounded once to `dtype`, component by component."""
    Tx, acc, peak = (_np(a) for a in got)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    assert Tx.dtype == np.dtype(cdt) and acc.dtype == np.int64, (name, Tx.dtype, acc.dtype)
    want_acc = ref['acc'].reshape(acc.shape)
    assert np.array_equal(peak.view(np.uint64), ref['peak']), (name, peak, ref['peak'])
    bad = acc != want_acc
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert int(np.abs(want_acc).max()) < 2 ** 62, name
    want = ref['Tx'].reshape(Tx.shape)
    assert np.array_equal(Tx.real, want.real.astype(dtype)) and np.array_equal(Tx.imag, want.imag.astype(dtype)), name


# ------------------------------------------------------------------------------------------ shapes and planes
def shapes(tr, tc, hc, wc, gcap, p):
    """(B, rows, n, top): `tr` x `tc` the tile of sources, `hc` the window's halo in columns, `wc` the window's columns,
    `gcap` the most workgroups of the windowed scatter, `p` the columns of `rot_lo`, as the library exports them; `top` the
    largest ``dmax[i]`` of `row_dmax`, or -1 for the bounds of `mixed_dmax`."""
    return [(1, 3, 1, 0),                         # one column
            (1, 1, wc + 40, 2 * hc),              # one row
            (1, tr - 1, tc - 1, 3),               # around the tile (and, the tile being p columns wide, around p)
            (1, tr, tc, 5),
            (1, tr + 1, tc + 1, 2 * hc),
            (1, 3, p - 1, 4), (1, 3, p, 4), (1, 3, p + 1, 4),
            (1, 3, 2 * p + 37, hc + 1),           # no multiple of p: three entries of rot_hi
            (3, 9, wc + 40, 2 * hc),              # batch: three shifts
            (2, 2, (gcap // 2 + 3) * tc - 5, 2 * hc),               # gcap + 6 tiles: some workgroups walk two
            (1, 6, wc + tc + 10, -1)]             # per-row bounds: 0, hc - 1, hc, hc + 1, > n, 3


SHAPE_IDS = ['one_column', 'one_row', 'tile_minus_1', 'tile', 'tile_plus_1', 'p_minus_1', 'p', 'p_plus_1', 'three_rot_hi',
             'batch', 'more_tiles_than_workgroups', 'mixed_bounds']
# the cases in which terms leave the window of their tile, whatever the library's sizes: the plane is wider than a window
# and a row's bound is twice the halo or more (a window that covers every column of the plane keeps every term, and so
# does a shift within the halo)
LEAVES = ('one_row', 'batch', 'more_tiles_than_workgroups', 'mixed_bounds')


def mixed_dmax(n, hc):
    return np.array([0, hc - 1, hc, hc + 1, n + 50, 3], dtype=np.int32)


def planes(shape, dtype, hc=64, seed=0):
    """Seeded ``(W, Wd, rsc, dmax, phi)``. `W` is standard normal, signal `b` of a batch scaled by ``10^(3 b)`` (so that
    `sh` differs per signal); ``Wd = W z`` with the displacements ``Im(z) rsc[i]`` spanning about 1.5 ``dmax[i]`` (two
    standard deviations): every drop branch is taken. `dmax` is `reassign_cwt.row_dmax` (or `mixed_dmax`), `rsc`
    proportional to it, `phi` the rows' frequencies, uniform in (0.01, 0.5) cycles per column."""
    B, rows, n, top = shape
    rng = np.random.default_rng([seed, B, rows, n, top + 1, 2019])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    amp = (10. ** (3 * np.arange(B)))[:, None, None]
    W = ((rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))) * amp).astype(cdt)
    dmax = mixed_dmax(n, hc) if top < 0 else RC.row_dmax(rows, top)
    if rows == 1:
        dmax = np.array([top], dtype=np.int32)                  # (a geometric rise of one row would stop at 1)
    assert len(dmax) == rows
    rsc = 3. * np.maximum(dmax, .5)
    z = rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))
    Wd = (W * (z * (.75 * dmax / rsc)[None, :, None])).astype(cdt)
    phi = rng.uniform(.01, .5, rows)
    return W, Wd, rsc, dmax, phi


def crafted(amp, d, rsc, dtype):
    """Planes that give chosen shifts exactly: ``W = amp`` (complex allowed), ``Wd = 1j (d / rsc[i]) W``; `amp` and `d`
    broadcast to one (B, rows, n) shape. ``Im(Wd / W) rsc[i]`` comes back within 1e-5 of the integer `d`."""
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    amp, d = np.broadcast_arrays(np.asarray(amp, dtype=np.complex128), np.asarray(d, dtype=np.float64))
    W = amp.astype(cdt)
    Wd = (W.astype(np.complex128) * (1j * d / np.asarray(rsc, dtype=np.float64)[None, :, None])).astype(cdt)
    return W, Wd


# ------------------------------------------------------------------------------------------ the whole transform
def design(wavelet, N, scales='log-piecewise', nv=16):
    """``(wav64, scales, freqs, dmax)`` of `tssq_cwt`'s defaults at fs = 1, the wavelet in float64."""
    from ssqueezepy_amd import algos
    from ssqueezepy_amd.wavelets import row_frequencies
    wav, sc, _, _, dmax = RC.design(wavelet, N, scales, nv)
    return wav, sc, row_frequencies(wav, sc, 1.), dmax


def np_tssq(x, wav, sc, phi, dmax, gamma):
    """``(Tx, W)`` of a 1-D signal in NumPy complex128: the planes of `reassign_cwt.np_planes`, the shift and the drop
    rules of `terms`, the rotation as a direct ``exp(-2j pi frac(phi c))`` and a float64 `np.add.at` (no fixed point, no
    tables: the restatement is of the transform, not of the sum)."""
    W, _, Wd = RC.np_planes(x, wav, sc)
    lands, c2, _, _, _, _ = terms(W[None], Wd[None], sc, dmax, None, gamma)
    n = W.shape[-1]
    z = W * np.exp(-2j * np.pi * np.mod(np.asarray(phi)[:, None] * np.arange(n)[None, :], 1.))
    Tx = np.zeros(W.shape, dtype=np.complex128)
    rows = np.broadcast_to(np.arange(W.shape[0])[:, None], W.shape)
    np.add.at(Tx, (rows[lands[0]], c2[0][lands[0]]), z[lands[0]])
    return Tx, W


def impulse(N):
    x = np.zeros(N)
    x[N // 2 - N // 9] = 1.
    return x, N // 2 - N // 9


def dispersive_pulse(N):
    """A pulse whose group delay rises linearly with frequency, ``tg(f) = 0.3 N + 0.4 N f / 0.5`` samples over 0.04 .. 0.46
    cycles per sample (flat spectrum, raised-cosine edges): returns ``(x, tg)``, `tg` a function of frequency."""
    f = np.fft.rfftfreq(N)
    a, b = .3 * N, .8 * N
    amp = np.clip((f - .04) / .04, 0., 1.) * np.clip((.46 - f) / .04, 0., 1.)
    amp = .5 - .5 * np.cos(np.pi * amp)
    x = np.fft.irfft(amp * np.exp(-2j * np.pi * (a * f + .5 * b * f * f)), N)
    return x / np.abs(x).max(), lambda fr: a + b * np.asarray(fr)


def share(E, tg, half):
    """The share of the plane `E` (rows, n), real and non-negative, within `half` columns of the column ``tg[i]`` of
    every row."""
    E = np.asarray(E, dtype=np.float64)
    c = np.arange(E.shape[1])[None, :]
    return float(E[np.abs(c - np.rint(np.asarray(tg))[:, None]) <= half].sum() / E.sum())


def e2e_case(kind, N):
    """``(x, wavelet, rows, tg, half)``: the signal, the wavelet, the rows read (centre frequency 0.06 .. 0.4 cycles per
    sample: wavelets that resolve and fit the signal), the true column of every such row, the half-width of the share."""
    wavelet = ('gmw', {'gamma': 3, 'beta': 60})
    _, sc, freqs, _ = design(wavelet, N)
    rows = np.flatnonzero((freqs >= .06) & (freqs <= .4))
    if kind == 'impulse':
        x, n0 = impulse(N)
        return x, wavelet, rows, np.full(len(rows), float(n0)), 1
    x, tg = dispersive_pulse(N)
    return x, wavelet, rows, tg(freqs[rows]), 3


_RESTATED = {}


def np_shares(kind, N):
    """``(share of |Tx|^2, share of the scalogram)`` from the restatement; computed once per case."""
    if (kind, N) not in _RESTATED:
        x, wavelet, rows, tg, half = e2e_case(kind, N)
        wav, sc, freqs, dmax = design(wavelet, N)
        Tx, W = np_tssq(x, wav, sc, freqs, dmax, 10 * EPS['float64'])
        _RESTATED[(kind, N)] = (share(np.abs(Tx[rows]) ** 2, tg, half), share(np.abs(W[rows]) ** 2, tg, half))
    return _RESTATED[(kind, N)]
