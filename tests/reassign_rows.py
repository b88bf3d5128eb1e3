# -*- coding: utf-8 -*-
"""Statements and inputs of the row-count tests of the reassignment kernels behind `launch_accumulate`
(csrc/ssq_kernels.hip): tests/test_reassign_rows_design.py (CPU), tests/test_gpu_reassign_rows.py (GPU) and
tests/test_reassign_rows_emulated.py (the same checks over the CPU emulation). NumPy only; no device code.

`route`        the routing rule restated from the LDS formulas -- a tile of `na` rows x `cols` columns of `cell`-byte
               cells against LDS_CAP (one workgroup per CU) and LDS_CAP / 2 (two) -- not from the C++.
`ordered_sum`  the reference's sum: rows ascending, the product and the sum in the CPU path's arithmetic.
`exact_sum`    per cell the number of terms, their exact sum and the sum of their magnitudes (np.longdouble).
`spread_case`  inputs whose bins cover the grid (see `spread_ok`); `PATTERNS` crafted bin maps; `int_plane` /
               `wide_plane` the two value families (order-free integer sums, order-sensitive magnitudes).
"""
import numpy as np
from conftest import make_ssq_freqs, const_of

LDS_CAP = 160 * 1024
SKIP = 0xFFFF
BINSRCS = ('dwx', 'w', 'bins')
GRIDS = ('log-piecewise', 'log', 'linear')
WEIGHTS = ('scalar', 'vecdt', 'vec64')
GAMMA = 1e-2

# both sides of every LDS edge and the RL, RL * U steps of each build (RL 8, U 3 / RL 16, U 4)
NAS = {'float32': (2, 7, 8, 9, 23, 24, 25, 320, 321, 1280, 1281, 2560, 2561, 5120, 5121),
       'float64': (2, 15, 16, 17, 63, 64, 65, 640, 641, 1280, 1281, 2560, 2561)}
# the documented limits: last row count of (tile16 32 columns, tile16 16, tile 8, tile 4); of the unordered float64 tile
ORDERED_LIMITS = {'float32': (320, 1280, 2560, 5120), 'float64': (640, 1280, 2560)}
F64_LIMITS = {'float32': (160, 640), 'float64': (160, 640, 1280)}
# the nine ordered builds: (dtype, kernel, cols, wavefronts) -> the first and the last row count that reaches it
BUILDS = {('float32', 'tile16', 32, 4): (1, 320), ('float32', 'tile16', 16, 2): (321, 1280),
          ('float32', 'tile', 8, 1): (1281, 2560), ('float32', 'tile', 4, 1): (2561, 5120),
          ('float32', 'global', 1, 4): (5121, None),
          ('float64', 'tile16', 16, 4): (1, 640), ('float64', 'tile', 8, 1): (641, 1280),
          ('float64', 'tile', 4, 1): (1281, 2560), ('float64', 'global', 1, 4): (2561, None)}
# the unordered float64 tile (bin map, default order): (dtype, cols) -> first and last row count
F64_BUILDS = {('float32', 32): (1, 160), ('float32', 16): (161, 640),
              ('float64', 32): (1, 160), ('float64', 16): (161, 640), ('float64', 8): (641, 1280)}


def cell_bytes(dtype):
    return 8 if np.dtype(dtype) == np.float32 else 16


def rows_that_fit(cols, cell, cap):
    """most rows of a tile of `cols` columns of `cell`-byte cells in `cap` bytes"""
    return cap // (cols * cell)


def route(dtype, binsrc, na, n, ordered=False, kmap=False):
    """(kernel, cols, wavefronts per workgroup) for a shape: the table of the issue, from the LDS formulas.
    kernel: 'tile16' (accumulate_tile16_kernel), 'tile' (accumulate_tile_kernel), 'f64' (accumulate_f64_kernel),
    'global' (accumulate_global_kernel)."""
    f32 = np.dtype(dtype) == np.float32
    cell = cell_bytes(dtype)
    short = na * n < 2 ** 31                      # the fast kernels index with 32 bits
    if binsrc == 'bins' and not ordered and not kmap and short:
        # float64 planes for both data types: 16 bytes per cell. 32 and 16 columns with two workgroups per CU, then 16
        # with one; 8 columns for float64 data only
        for cols, cap in ((32, LDS_CAP // 2), (16, LDS_CAP // 2), (16, LDS_CAP)) + (() if f32 else ((8, LDS_CAP),)):
            if na <= rows_that_fit(cols, 16, cap):
                return 'f64', cols, 8
    if short and na <= rows_that_fit(16, cell, LDS_CAP):
        if not f32:
            return 'tile16', 16, 4                # 16 row-lanes x 4 columns per wavefront
        if na <= rows_that_fit(32, cell, LDS_CAP // 2):
            return 'tile16', 32, 4                # 8 row-lanes x 8 columns per wavefront
        return 'tile16', 16, 2
    for cols, cap in ((16, LDS_CAP // 2), (8, LDS_CAP // 2), (16, LDS_CAP), (8, LDS_CAP), (4, LDS_CAP)):
        if na <= rows_that_fit(cols, cell, cap):
            return 'tile', cols, 1
    return 'global', 1, 4


def query(A, dtype, binsrc, na, n, ordered=False, kmap=False):
    """`ssq_reassign_route` through `algos.reassign_route`."""
    return A.reassign_route(dtype, binsrc, na, n, ordered=ordered, kmap=kmap)


def row_lanes(dtype, kernel, cols):
    """rows a wavefront step covers per column (RL; 64 / cols for the one-wavefront tile)"""
    if kernel == 'tile16':
        return 8 if np.dtype(dtype) == np.float32 else 16
    return 64 // cols if kernel in ('tile', 'f64') else 1


# ---------------------------------------------------------------------------------------------- the two references
def weights_of(const, na, dtype):
    """The per-row weight vector and whether the product is formed in double (float32 data, float64 vector): what
    `algos._const_vector` and the oracle's `_const_vec` make."""
    f32 = np.dtype(dtype) == np.float32
    c = np.asarray(const)
    if c.size != na:
        return np.full(na, float(c), dtype=dtype), False
    c = c.reshape(-1)
    if f32 and c.dtype == np.float64:
        return c, True
    return c.astype(dtype), False


def _planes(Wx):
    return np.ascontiguousarray(Wx.real), np.ascontiguousarray(Wx.imag)


def ordered_sum(Wx, k, const):
    """``Tx[k[i, j], j] += Wx[i, j] * const[i]`` for ascending `i` (``k < 0`` = skip), real and imaginary part on
    their own, in the CPU path's arithmetic: float32 data with a float32 weight all in float32; float32 data with a
    float64 weight ``(float32)((double)o + (double)z * w)``; float64 data all in float64."""
    na, n = Wx.shape
    rdt = Wx.real.dtype
    w, wide = weights_of(const, na, rdt)
    out = [np.zeros((na, n), rdt), np.zeros((na, n), rdt)]
    cols = np.arange(n)
    for i in range(na):
        live = k[i] >= 0
        if not live.any():
            continue
        jj, kk = cols[live], k[i][live]
        for o, z in zip(out, _planes(Wx[i])):
            if wide:
                o[kk, jj] = (o[kk, jj].astype(np.float64) + z[jj].astype(np.float64) * w[i]).astype(rdt)
            else:
                o[kk, jj] = o[kk, jj] + z[jj] * w[i]
    return (out[0] + 1j * out[1]).astype(Wx.dtype)


def exact_sum(Wx, k, const):
    """Per cell: `m` the number of terms (int, (na, n)); `S` their exact sum and `A` the sum of their magnitudes, each a
    pair (real, imaginary) of np.longdouble planes. A term is formed as the kernels form it (`Term::make`): the
    float32 product for float32 data with a float32 weight, else the float64 product."""
    na, n = Wx.shape
    rdt = Wx.real.dtype
    w, wide = weights_of(const, na, rdt)
    m = np.zeros((na, n), np.int64)
    S = [np.zeros((na, n), np.longdouble), np.zeros((na, n), np.longdouble)]
    A = [np.zeros((na, n), np.longdouble), np.zeros((na, n), np.longdouble)]
    cols = np.arange(n)
    for i in range(na):
        live = k[i] >= 0
        if not live.any():
            continue
        jj, kk = cols[live], k[i][live]
        m[kk, jj] += 1
        for s, a, z in zip(S, A, _planes(Wx[i])):
            t = (z[jj].astype(np.float64) * w[i]) if wide else (z[jj] * w[i])
            t = t.astype(np.longdouble)
            s[kk, jj] += t
            a[kk, jj] += np.abs(t)
    return m, S, A


def f64_sum_bound(dtype, m, S, A):
    """The rounding bound of a float64 sum of `m` terms in any order, plus one rounding to float32 for float32 data:
    ``m 2^-53 A`` and ``m 2^-53 A + 2^-24 (|S| + m 2^-53 A)``, one plane."""
    b = m.astype(np.longdouble) * np.longdouble(2.0 ** -53) * A
    if np.dtype(dtype) == np.float32:
        b = b + np.longdouble(2.0 ** -24) * (np.abs(S) + b)
    return b


def to_map(k):
    """int bins (< 0 = skip) -> the uint16 map of `indexed_sum_bins`"""
    return np.where(k < 0, SKIP, k).astype(np.uint16)


# ---------------------------------------------------------------------------------------------- spread inputs
def grid_params(sf, grid):
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    return ssq_grid_params(sf, grid.startswith('log'))[1]


def columns_for(na):
    """columns of the row-count cases: past two 32-column tiles, odd, and enough points per bin for `spread_ok`"""
    return 70 if na <= 1281 else 45


def spread_case(dtype, na, n, grid, seed=0, stft=False):
    """`Wx`, `dWx`, `gamma` (and `Sfs` with `stft`) whose bins spread over the grid: `Wx` random with per-column
    distinct values, ``dWx = Wx 2 pi i f`` with `f` log-uniform over the grid's span (uniform on the linear grid), 5 %
    of the points below the first bin (the linear grid starts at 0 and the bin is taken of ``|f|``: there inside the
    first half bin), 5 % above the last; a few points below `gamma`, one `Wx` and one `dWx` exactly 0."""
    rng = np.random.default_rng(1000 * seed + na + (7 if stft else 0) + 13 * GRIDS.index(grid))
    cdt = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    Sfs = np.linspace(0, .5, na).astype(dtype) if stft else None
    sf = (Sfs if stft else make_ssq_freqs(na, grid)).astype(np.float64)      # (the STFT form bins on Sfs itself)
    Wx = ((rng.standard_normal((na, n)) + 1j * rng.standard_normal((na, n))) * (1 + np.arange(n) / n)).astype(cdt)
    u = rng.random((na, n))
    if grid == 'linear':
        f = u * sf[-1]
        lo, hi = rng.random((na, n)) * 0.4 * (sf[1] - sf[0]), sf[-1] * (1.05 + rng.random((na, n)))
    else:
        f = np.exp(np.log(sf[0]) + u * (np.log(sf[-1]) - np.log(sf[0])))
        lo, hi = sf[0] * (0.1 + 0.8 * rng.random((na, n))), sf[-1] * (1.05 + rng.random((na, n)))
    side = rng.random((na, n))
    f = np.where(side < 0.05, lo, np.where(side > 0.95, hi, f))
    if stft:
        f = Sfs[:, None].astype(np.float64) - f             # w = |Sfs - Im(dSx / Sx) / 2 pi| = |f| again
    dWx = (Wx.astype(np.complex128) * (2j * np.pi * f)).astype(cdt)
    flat = rng.permutation(na * n)[:8]
    Wx.reshape(-1)[flat[:5]] *= 1e-4                        # below gamma
    Wx.reshape(-1)[flat[5]] = 0
    dWx.reshape(-1)[flat[6]] = 0
    return dict(Wx=Wx, dWx=dWx, Sfs=Sfs, gamma=GAMMA, sf=make_ssq_freqs(na, grid) if not stft else Sfs, grid=grid)


def w_plane(orc, case):
    """the matching `w` plane: the oracle's phase transform (inf below gamma) with a few more inf"""
    c = case
    if c['Sfs'] is not None:
        w = orc.phase_stft(c['Wx'], c['dWx'], c['Sfs'], c['gamma'], typing=0)
    else:
        w = orc.phase_cwt(c['Wx'], c['dWx'], c['gamma'], typing=0)
    w = w.copy()
    w.reshape(-1)[::max(1, w.size // 5) + 1] = np.inf
    return w


def spread_bound(na):
    """The largest share of the points one bin may hold: 10 %. With fewer than 18 bins that cannot be met -- the two
    clamps hold 5 % each by construction and an even spread leaves 0.9 / na per bin -- so there the bound is the
    clamp's 5 % plus twice the even share."""
    return max(0.10, 0.05 + 2 * 0.9 / na)


def spread_ok(kmap, na):
    """(share of the bins that receive a point, largest share of the points in one bin) of an int bin map"""
    k = kmap[kmap >= 0]
    cnt = np.bincount(k, minlength=na)
    return float((cnt > 0).mean()), float(cnt.max() / max(1, k.size))


# ---------------------------------------------------------------------------------------------- crafted bin maps
def _rows(na, n, f):
    i = np.arange(na)[:, None] + np.zeros((1, n), np.int64)
    return np.asarray(f(i), dtype=np.int64)


def _gaps(na):
    def f(i):
        far = (3 * i + 1) % na                              # rows of other bins between the matches
        return np.where(i % 3 == 0, min(5, na - 1), np.where(i % 3 == 1, -1, far))
    return f


def _period(p, na):
    def f(i):
        return np.where(i % p == 0, min(3, na - 1), i % na)
    return f


def _colmix(na, n):
    i, j = np.arange(na)[:, None], np.arange(n)[None, :]
    return (i // (1 + j % 4) + 5 * (j % 3)) % na


def patterns(na, n):
    """name -> int (na, n) bin map, < 0 = skip. All but 'colmix' give every column the same bins, so that with data that
    differ per column a term that leaks into a neighbouring column of the same DPP row shows."""
    P = {'all_to_0': _rows(na, n, lambda i: 0 * i),
         'all_to_mid': _rows(na, n, lambda i: 0 * i + na // 2),
         'all_to_last': _rows(na, n, lambda i: 0 * i + na - 1),
         'identity': _rows(na, n, lambda i: i),
         'reversed': _rows(na, n, lambda i: na - 1 - i),
         'halves': _rows(na, n, lambda i: i // 2),
         'mod2': _rows(na, n, lambda i: i % 2 % na),
         'mod3': _rows(na, n, lambda i: i % 3 % na),
         'gaps': _rows(na, n, _gaps(na)),
         'period9': _rows(na, n, _period(9, na)),           # RL + 1 of the 8-lane builds
         'period17': _rows(na, n, _period(17, na)),         # RL + 1 of the 16-lane builds
         'colmix': _colmix(na, n)}
    for k in P.values():
        assert k.shape == (na, n) and k.max() < na
    return P


PATTERN_NAMES = tuple(patterns(20, 3))
ORDER_FREE = ('identity', 'reversed', 'halves')       # one or two terms per cell: the sum does not depend on the order


PATTERN_GAMMA = 1e-12       # below every value of `wide_plane` (2^-20 times a normal deviate), above the skipped points' 0


def pattern_planes(Wx, k, sf):
    """A crafted map as the inputs of the other two bin sources on the linear grid `sf`: ``w = sf[k]`` (inf = skip) and
    ``dWx = Wx 2 pi i sf[k]`` with `Wx` set to 0 where the map skips (`PATTERN_GAMMA` drops those). -> (w, dWx, Wx)"""
    rdt = Wx.real.dtype
    f = np.asarray(sf, dtype=np.float64)[np.maximum(k, 0)]
    w = np.where(k < 0, np.inf, f).astype(rdt)
    Wz = np.where(k < 0, 0, Wx).astype(Wx.dtype)
    dWx = (Wz.astype(np.complex128) * (2j * np.pi * f)).astype(Wx.dtype)
    return w, dWx, Wz


def int_plane(dtype, na, n, seed=1):
    """Integer-valued `Wx` (|re|, |im| <= 2^10, smaller for tall planes) and a power-of-two weight vector: every
    partial sum of a column is an integer multiple of 1/4 below 2^24 of them, so float32 and float64 sums are exact
    in any order."""
    rng = np.random.default_rng(seed + na)
    V = int(min(2 ** 10, 2 ** 21 // na))
    cdt = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    Wx = (rng.integers(-V, V + 1, (na, n)) + 1j * rng.integers(-V, V + 1, (na, n))).astype(cdt)
    w = (2.0 ** (np.arange(na) % 3 - 1)).astype(dtype)      # 1/2, 1, 2
    assert na * V * 2 * 2 < 2 ** 24
    return Wx, w


def wide_plane(dtype, na, n, seed=2):
    """`Wx` with magnitudes spread over 2^-20 .. 2^20: sums in the data type depend on the order of the additions."""
    rng = np.random.default_rng(seed + na)
    cdt = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    mag = 2.0 ** rng.uniform(-20, 20, (na, n))
    return ((rng.standard_normal((na, n)) + 1j * rng.standard_normal((na, n))) * mag).astype(cdt)


def weight(kind, na, dtype):
    """'scalar' | 'vecdt' | 'vec64' (conftest.const_of: 'vecdt' in the data type, 'vec64' float64 for both)"""
    return const_of(kind, na, dtype)
