# -*- coding: utf-8 -*-
"""What the tests of `ssq_conceft_cwt` share (tests/test_gpu_conceft_cwt.py and its emulated twin): the NumPy
statement of the entry (include/ssq_hip.h) and the columns it leaves out.

As in tests/conceft.py the statement works on separate real float64 arrays with one ufunc per operation, in the
stated order; `mix`, `unit_rows`, `clamp_round` and `check` are that module's. What is new here: no `Sfs` in the
phase, a weight `cst[i]` on every term, and the three bin maps. The log maps go through `log2(w)`, where the device's
`log2` and NumPy's may differ by an ulp: a column in which some point's fractional bin position lies within 1e-9 of a
rounding boundary (an ulp of `log2 w` moves it by about 1e-13 on these grids) is left out, next to the columns with a
point near `gamma`.
"""
import numpy as np
from conceft import mix, unit_rows, clamp_round, check, above_median, near_gamma_columns, magnitudes, _np, EPS64, TWO_PI  # noqa: F401

# (B, J, Q, rows, n)
SHAPES = [(1, 1, 1, 5, 7),         # smallest case
          (2, 3, 4, 33, 50),       # n not a multiple of any tile width, and a second signal
          (1, 8, 17, 65, 19),      # largest J, odd Q
          (1, 2, 3, 272, 37),      # the last row count of the 17-cell build ...
          (1, 2, 3, 273, 37),      # ... and the first of the 40-cell build
          (1, 2, 2, 640, 19),      # the last row count of the 16-column tile ...
          (1, 2, 2, 641, 9),       # ... and the first of the 8-column tile
          (1, 2, 2, 1280, 9)]      # the most rows the entry takes
GRIDS = ['linear', 'log', 'log-piecewise']
F_LO, F_HI = 2., 32.               # the grids' ends
W_MID = 8.                         # where the median of `w` is put: 2 octaves from either end
NEAR_BOUNDARY = 1e-9
# The seed of a shape's planes, 0 unless listed: the smallest with which the statement leaves out no column on any grid
# in either dtype and bin 0, the top bin and an interior bin all receive points (tests/test_conceft_cwt_emulated.py
# checks the first, test_kernel_vs_statement the second). With seed 0 the 17 points that the smallest shape keeps miss
# the top bin, and in the 272-row shape the two samples of |Wq| that `gamma` is put between lie 1.2e-6 (relative)
# apart, so both count as near `gamma`: 2 of 37 columns.
SEEDS = {(1, 1, 1, 5, 7): 7, (1, 2, 3, 272, 37): 1}


def ssq_freqs(kind, rows):
    """The grid of `rows` bins from `F_LO` to `F_HI`, float64: linear, exponential (``2**linspace``), or exponential
    in two pieces -- the lower half of the rows over the lowest octave, the rest over the other three."""
    if kind == 'linear':
        return np.linspace(F_LO, F_HI, rows)
    lo, hi = np.log2(F_LO), np.log2(F_HI)
    if kind == 'log':
        return 2. ** np.linspace(lo, hi, rows)
    r0 = rows // 2 + 1
    return 2. ** np.concatenate([np.linspace(lo, lo + 1, r0, endpoint=False), np.linspace(lo + 1, hi, rows - r0)])


def planes(shape, dtype, seed=None):
    """Seeded standard-normal planes `W`, `dW` (J, B, rows, n), unit projections (Q, J) and positive random weights
    `cst` (rows,) float64. `dW` is scaled so that the median of ``w = |Im(dWq / Wq)| / 2pi`` is about `W_MID`
    (``|Im(dWq / Wq)|`` of two independent standard complex normals has median ``1 / sqrt(3)``): `w` spans the
    grids and leaves them at both ends."""
    B, J, Q, rows, n = shape
    seed = SEEDS.get(tuple(shape), 0) if seed is None else seed
    rng = np.random.default_rng([seed, B, J, Q, rows, n, 2016])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    W, dW = [(rng.standard_normal((J, B, rows, n)) + 1j * rng.standard_normal((J, B, rows, n))).astype(cdt)
             for _ in range(2)]
    dW = dW * cdt(W_MID * TWO_PI * np.sqrt(3.))
    proj = unit_rows(rng.standard_normal((Q, J)) + 1j * rng.standard_normal((Q, J)))
    cst = rng.uniform(.5, 2., rows)
    return W, dW, proj, cst


def bins(w, kind, p, omax):
    """``(k, near)``: `bin_from_w` (csrc/ssq_point_math.inl) in NumPy, before `flipud`, and whether the point's
    fractional bin position lies within `NEAR_BOUNDARY` of a rounding boundary (or of the seam of the two pieces)."""
    from ssqueezepy_amd.ssqueezing import GRID_LIN, GRID_LOG
    p = [float(v) for v in p]

    def frac_near(t):
        return (np.abs(np.subtract(t, np.floor(t)) - .5) < NEAR_BOUNDARY) & (t > 0) & (t < omax)
    with np.errstate(all='ignore'):
        if kind == GRID_LIN:
            t = np.divide(np.subtract(w, p[0]), p[1])
            return clamp_round(t, omax), frac_near(t)
        wl = np.log2(w)
        if kind == GRID_LOG:
            t = np.divide(np.subtract(wl, p[0]), p[1])
            return clamp_round(t, omax), frac_near(t)
        upper = wl > p[1]
        tu = np.divide(np.subtract(wl, p[1]), p[3])
        ku = np.where(tu < 4.0e18, np.rint(np.where(tu < 4.0e18, tu, 0.)) + np.trunc(p[4]), omax)
        ku = np.clip(ku, 0, omax).astype(np.int64)
        tl = np.divide(np.subtract(wl, p[0]), p[2])
        k = np.where(upper, ku, clamp_round(tl, omax))
        near = np.where(upper, (np.abs(np.subtract(tu, np.floor(tu)) - .5) < NEAR_BOUNDARY) & (tu + p[4] < omax),
                        frac_near(tl)) | (np.abs(np.subtract(wl, p[1])) < NEAR_BOUNDARY)
        return k, near


def projections(W, dW, cst, proj, gamma, freqs):
    """``(Tr, Ti, near)``: every `Tq` of the statement before `flipud`, (Q, B, rows, n) float64 each, and the
    (B, n) columns with a point near a rounding boundary."""
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    from ssqueezepy_amd.scales import infer_scaletype
    kind, p = ssq_grid_params(freqs, infer_scaletype(np.asarray(freqs))[0].startswith('log'))
    J, B, rows, n = W.shape
    omax = rows - 1
    cst = np.broadcast_to(np.asarray(cst, dtype=np.float64).reshape(-1), (rows,))
    Tr, Ti = np.zeros((len(proj), B, rows, n)), np.zeros((len(proj), B, rows, n))
    near = np.zeros((B, n), dtype=bool)
    for q, r in enumerate(proj):
        vr, vi = mix(W, r)
        dr, di = mix(dW, r)
        for i in range(rows):
            a, b, c, d = dr[:, i], di[:, i], vr[:, i], vi[:, i]
            keep = ~(np.hypot(c, d) < gamma)
            with np.errstate(all='ignore'):
                num = np.subtract(np.multiply(b, c), np.multiply(a, d))
                den = np.multiply(np.add(np.multiply(c, c), np.multiply(d, d)), TWO_PI)
                w = np.abs(np.divide(num, den))
            k, nb = bins(w, kind, p, omax)
            near |= nb & keep
            bb, cc = np.nonzero(keep)               # one point per (signal, column): no index repeats
            Tr[q, bb, k[bb, cc], cc] += np.multiply(c, cst[i])[bb, cc]
            Ti[q, bb, k[bb, cc], cc] += np.multiply(d, cst[i])[bb, cc]
    return Tr, Ti, near


def average_of(Tr, Ti, flipud=False, average='abs'):
    """`Cx` in float64 (complex128 for ``average='complex'``), not yet rounded to an output dtype, from
    `projections`' `Tq`: ``flipud`` sends bin `k` to ``rows-1-k`` (a cell keeps its terms and their order)."""
    if flipud:
        Tr, Ti = Tr[:, :, ::-1], Ti[:, :, ::-1]
    acc_r, acc_i = np.zeros(Tr.shape[1:]), np.zeros(Tr.shape[1:])
    for q in range(len(Tr)):
        if average == 'abs':
            acc_r = np.add(acc_r, np.hypot(Tr[q], Ti[q]))
        else:
            acc_r, acc_i = np.add(acc_r, Tr[q]), np.add(acc_i, Ti[q])
    Q = float(len(Tr))
    return np.divide(acc_r, Q) if average == 'abs' else np.divide(acc_r, Q) + 1j * np.divide(acc_i, Q)


def statement(W, dW, cst, proj, gamma, freqs, flipud=False, average='abs'):
    Tr, Ti, _ = projections(W, dW, cst, proj, gamma, freqs)
    return average_of(Tr, Ti, flipud, average)


def check_cwt(name, Cx_dev, ref, near, Q, dtype, average):
    """`conceft.check` with the float64 'abs' bound of this entry, ``(5 + Q) eps |statement|``: one more rounding
    than the STFT form's ``(4 + Q)``, for the weight."""
    return check(name, Cx_dev, ref, near, Q + 1, dtype, average)
