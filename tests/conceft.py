# -*- coding: utf-8 -*-
"""What the tests of `ssq_conceft` share (tests/test_gpu_conceft.py and its emulated twin): the NumPy statement
of the entry (include/ssq_hip.h) and the comparison of a device result with it.

The statement works on separate real float64 arrays with one ufunc per operation, in the stated order: NumPy's
complex multiply may fuse a product into a sum, real ufuncs cannot. Loops over `q`, `i` and `j` are Python loops;
the columns (and signals) of a row are independent and go through the ufuncs together.
"""
import numpy as np

TWO_PI = 6.283185307179586
EPS64 = float(np.finfo(np.float64).eps)
# (B, J, Q, rows, n)
SHAPES = [(1, 1, 1, 5, 7),         # smallest case
          (2, 3, 4, 33, 50),       # n not a multiple of any tile width, and a second signal
          (1, 8, 17, 65, 19),      # largest J, odd Q
          (1, 2, 3, 257, 37),      # a tile with spare columns at the edge
          (1, 2, 2, 513, 19),      # rows at the widest-tile limit
          (1, 2, 2, 1025, 9)]      # the narrow tile
FS = 200.


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def above_median(v):
    """Midway between the median sample and the next one up (`second_order._above_median`)."""
    v = np.sort(np.asarray(v, dtype=np.float64).reshape(-1))
    k = len(v) // 2
    return .5 * (v[k] + v[k + 1])


def unit_rows(z):
    z = np.asarray(z, dtype=np.complex128)
    return z / np.sqrt((z.real ** 2 + z.imag ** 2).sum(axis=1, keepdims=True))


def planes(shape, dtype, seed=0):
    """Seeded standard-normal planes `V`, `dV` (J, B, rows, n), unit projections (Q, J) and `Sfs`."""
    B, J, Q, rows, n = shape
    rng = np.random.default_rng([seed, B, J, Q, rows, n])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    V, dV = [(rng.standard_normal((J, B, rows, n)) + 1j * rng.standard_normal((J, B, rows, n))).astype(cdt)
             for _ in range(2)]
    dV = (dV * cdt(.25 * FS))                  # derivative planes: the phase term spans the grid and leaves it
    proj = unit_rows(rng.standard_normal((Q, J)) + 1j * rng.standard_normal((Q, J)))
    return V, dV, proj, np.linspace(0, .5 * FS, rows).astype(dtype)


def mix(P, r):
    """``sum_j r[j] P[j]`` from 0 in ascending j, real and imaginary sums separate, float64."""
    sr, si = np.zeros(P.shape[1:]), np.zeros(P.shape[1:])
    for j in range(len(P)):
        ar, ai = float(r[j].real), float(r[j].imag)
        pr, pi = P[j].real.astype(np.float64), P[j].imag.astype(np.float64)
        sr = np.add(sr, np.subtract(np.multiply(ar, pr), np.multiply(ai, pi)))
        si = np.add(si, np.add(np.multiply(ar, pi), np.multiply(ai, pr)))
    return sr, si


def magnitudes(V, proj):
    """``hypot(Vq)`` of every projection: (Q, B, rows, n)."""
    return np.stack([np.hypot(*mix(V, r)) for r in proj])


def clamp_round(t, omax):
    with np.errstate(invalid='ignore'):
        k = np.where(t > 0, np.minimum(np.rint(np.where(np.isfinite(t), t, 0.)), omax), 0.)
        k = np.where(t >= omax, omax, k)
    return k.astype(np.int64)


def statement(V, dV, Sfs, proj, gamma, ssq_freqs, flipud=False, average='abs'):
    """`Cx` in float64 (complex128 for ``average='complex'``), not yet rounded to an output dtype: (B, rows, n)."""
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    _, p = ssq_grid_params(ssq_freqs, False)
    p0, p1 = float(p[0]), float(p[1])
    J, B, rows, n = V.shape
    omax = rows - 1
    Sfs = np.asarray(Sfs).astype(np.float64)
    acc_r, acc_i = np.zeros((B, rows, n)), np.zeros((B, rows, n))
    for r in proj:
        vr, vi = mix(V, r)
        dr, di = mix(dV, r)
        Tr, Ti = np.zeros((B, rows, n)), np.zeros((B, rows, n))
        for i in range(rows):
            a, b, c, d = dr[:, i], di[:, i], vr[:, i], vi[:, i]
            keep = ~(np.hypot(c, d) < gamma)
            with np.errstate(all='ignore'):
                num = np.subtract(np.multiply(b, c), np.multiply(a, d))
                den = np.multiply(np.add(np.multiply(c, c), np.multiply(d, d)), TWO_PI)
                w = np.abs(np.subtract(Sfs[i], np.divide(num, den)))
                k = clamp_round(np.divide(np.subtract(w, p0), p1), omax)
            if flipud:
                k = omax - k
            bb, cc = np.nonzero(keep)               # one point per (signal, column): no index repeats
            Tr[bb, k[bb, cc], cc] += c[bb, cc]
            Ti[bb, k[bb, cc], cc] += d[bb, cc]
        if average == 'abs':
            acc_r = np.add(acc_r, np.hypot(Tr, Ti))
        else:
            acc_r, acc_i = np.add(acc_r, Tr), np.add(acc_i, Ti)
    Q = float(len(proj))
    return np.divide(acc_r, Q) if average == 'abs' else np.divide(acc_r, Q) + 1j * np.divide(acc_i, Q)


def near_gamma_columns(mags, gamma):
    """(B, n): the columns in which some ``|hypot(Vq) - gamma| <= 1e-6 gamma`` -- the device's `hypot` and libm's
    may put such a point on different sides."""
    return (np.abs(mags - gamma) <= 1e-6 * gamma).any(axis=(0, 2))


def check(name, Cx_dev, ref, near, Q, dtype, average):
    """The device's `Cx` (B, rows, n) against the statement on the columns kept; returns the worst ratio of error to
    bound. float32: within one `np.spacing` of the statement rounded to float32. float64, 'abs': within
    ``(4 + Q) eps |statement|`` -- bins and sum order are identical, the device's and libm's `hypot` may differ by an
    ulp per term and the Q additions round separately. 'complex': equal. An empty cell is exactly 0; no NaN anywhere."""
    from conftest import report_measured
    Cx_dev = _np(Cx_dev)
    cplx = average == 'complex'
    rdt = np.dtype(dtype)
    assert Cx_dev.shape == ref.shape, (name, Cx_dev.shape, ref.shape)
    assert Cx_dev.dtype == (np.result_type(rdt, np.complex64) if cplx else rdt), (name, Cx_dev.dtype)
    assert not np.isnan(Cx_dev).any(), name
    assert near.mean() <= .01, (name, float(near.mean()))
    keep = np.broadcast_to(~near[:, None, :], ref.shape)
    want = ref.astype(Cx_dev.dtype)
    empty = keep & (ref == 0)
    assert (Cx_dev[empty] == 0).all(), name
    ratio = 0.
    if cplx:
        assert np.array_equal(Cx_dev[keep], want[keep]), (name, int((Cx_dev[keep] != want[keep]).sum()))
    else:
        err = np.abs(Cx_dev.astype(np.float64) - want.astype(np.float64))[keep]
        bound = (np.spacing(np.abs(want)).astype(np.float64) if rdt == np.float32 else (4 + Q) * EPS64 * np.abs(ref))[keep]
        nz = bound > 0
        assert (err[~nz] == 0).all(), name
        ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.
        report_measured(name, max_err_over_bound=ratio, excluded_columns=int(near.sum()),
                        filled=float((ref != 0).mean()))
        assert (err <= bound).all(), (name, ratio)
    return ratio
