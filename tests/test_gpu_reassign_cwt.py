# -*- coding: utf-8 -*-
"""`reassign_cwt`, `algos.reassign_cwt_gpu` and the entry `ssq_reassign_cwt` (the reassigned scalogram: a fixed-point
scatter to the bin of the instantaneous frequency and to the group delay).

The oracle of the kernels is `reassign_cwt.statement`: the entry's definition in NumPy on separate real float64 arrays,
one ufunc per operation, the sum as `np.add.at` on uint64. The sum is an integer sum and the definition has basic IEEE
operations only, but for the `log2` of the two log grids and the `hypot` of float64 planes: `acc`, `peak` and `Rx` are
compared with `==` in both dtypes, and every seeded case asserts that the statement reports no point within 1e-9 of a
rounding boundary of the bin map and none within 1e-6 (relative) of `gamma` -- nothing is left out of the comparison.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import reassign2d as R
import reassign_cwt as Q
from reassign_cwt import _np

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
GRIDS = Q.GRIDS
SHAPE_IDS = Q.SHAPE_IDS
BATCH, SCATTERED, TILE_PLUS_1 = SHAPE_IDS.index('batch'), SHAPE_IDS.index('scattered'), SHAPE_IDS.index('tile_plus_1')


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def tile():
    """(tile rows, tile columns, halo bins, halo columns, most workgroups, window bins, window columns) of the library
    in use."""
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    return tuple(lib.ssq_reassign_cwt_tile(i) for i in range(7))


def shape_of(idx):
    shapes = Q.shapes(*tile())
    assert len(shapes) == len(SHAPE_IDS)
    return shapes[idx]


_CASES, _REFS = {}, {}


def case(shape, dtype):
    """Planes, row vectors and a `gamma` midway between two neighbouring samples of ``|W|`` near the lower quartile of
    the smallest signal; made once, nobody writes to them."""
    key = (shape, dtype)
    if key not in _CASES:
        W, dW, Wd, cst, rsc, dmax = Q.planes(shape, dtype)
        _CASES[key] = (W, dW, Wd, cst, rsc, dmax, R.quiet_gamma(W))
    return _CASES[key]


def reference(shape, dtype, kind='log', flipud=False, freq=True, time=True):
    key = (shape, dtype, kind if freq else None, flipud and freq, freq, time)
    if key not in _REFS:
        W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
        _REFS[key] = Q.statement(W, dW if freq else None, Wd if time else None, cst, rsc, dmax,
                                 Q.C.ssq_freqs(kind, shape[1]), gamma, flipud)
    return _REFS[key]


def run(S, W, dW, Wd, cst, rsc, dmax, freqs, gamma, **kw):
    return S.reassign_cwt_gpu(W, dW, Wd, rsc, cst, dmax, freqs, gamma, return_acc=True, **kw)


def run_case(S, shape, dtype, kind='log', flipud=False, freq=True, time=True, **kw):
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
    return run(S, W, dW if freq else None, Wd if time else None, cst, rsc, dmax, Q.C.ssq_freqs(kind, shape[1]), gamma,
               flipud=flipud, **kw)


def scattered_home(rows):
    """Homes all over the place and beyond: a permutation of the rows stretched over five times the grid."""
    return np.random.default_rng(3).permutation(rows) * 5 - 2 * rows


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def sync():
    import torch
    torch.cuda.synchronize() if DEV == 'cuda' else None


def same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ kernels against statement
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('flipud', [False, True], ids=['', 'flipud'])
@pytest.mark.parametrize('kind', GRIDS)
@pytest.mark.parametrize('idx', range(len(SHAPE_IDS)), ids=SHAPE_IDS)
def test_kernel_vs_statement(S, idx, kind, flipud, dtype):
    from ssqueezepy_amd import algos
    tr, tc, hr, hc, gcap, wr, wc = tile()
    shape = shape_of(idx)
    B, rows, n, top = shape
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
    freqs = Q.C.ssq_freqs(kind, rows)
    ref = reference(shape, dtype, kind, flipud)
    assert ref['near_boundary'] == 0 and ref['near_gamma'] == 0         # the condition the equalities rest on
    lands = ref['lands']
    if n > 1:
        assert 0 < lands.mean() < 1                         # some points are dropped, some land
    if B > 1:
        assert len(set(ref['sh'])) == B                     # a shift per signal
    if rows > 4 and kind != 'linear':
        k2 = ref['k2'][lands]
        assert (k2 == 0).any() and (k2 == rows - 1).any() and ((k2 > 0) & (k2 < rows - 1)).any()      # both end bins
    home = scattered_home(rows) if idx == SCATTERED else algos.reassign_cwt_home(rsc, freqs, flipud)
    # the share of the landing terms that leave the window of their tile (bins and columns)
    k = np.arange(rows)
    hmin = np.array([home[i // tr * tr:i // tr * tr + tr].min() for i in k])[None, :, None]
    c = np.arange(n)[None, None, :]
    out = (ref['k2'] < hmin - hr) | (ref['k2'] >= hmin - hr + wr) | (ref['c2'] < c // tc * tc - hc) | \
        (ref['c2'] >= c // tc * tc - hc + wc)
    outside = float((out & lands).sum() / max(lands.sum(), 1))
    if SHAPE_IDS[idx] == 'more_tiles_than_workgroups':
        assert B * -(-rows // tr) * -(-n // tc) > gcap
    if idx == SCATTERED:
        assert outside > .5
    got = run(S, W, dW, Wd, cst, rsc, dmax, freqs, gamma, flipud=flipud, home=home if idx == SCATTERED else None)
    Q.check('reassign_cwt_%s_%s_%d_%s' % (SHAPE_IDS[idx], kind, flipud, dtype), got, ref, dtype)
    report_measured('reassign_cwt_kernel_%s_%s_%d_%s' % (SHAPE_IDS[idx], kind, flipud, dtype), landed=float(lands.mean()),
                    outside_window=outside, filled=float((ref['acc'] != 0).mean()))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('freq,time', [(True, False), (False, True), (False, False)], ids=['freq', 'time', 'neither'])
def test_modes(S, freq, time, dtype):
    """Each axis alone, and both off: the statement's bits; with both off `Rx` is ``|W|^2 cst[i]`` in its own cell, to
    the fixed-point bound."""
    shape = shape_of(BATCH)
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
    for kind, flipud in (('log-piecewise', True), ('linear', False)):
        ref = reference(shape, dtype, kind, flipud, freq, time)
        got = run_case(S, shape, dtype, kind, flipud, freq, time)
        Q.check('reassign_cwt_mode_%d%d_%s' % (freq, time, dtype), got, ref, dtype)
        assert ref['C'] == Q.cell_terms(dmax, shape[2], freq, time)
        if not time:
            assert (ref['c2'] == np.arange(shape[2])[None, None, :]).all()
        if not freq:
            assert (ref['k2'] == np.arange(shape[1])[None, :, None]).all()      # (flipud mirrors bins, not rows)
    if not freq and not time:
        e, kept = R.energy(W, gamma)
        want = np.where(kept, e * cst[None, :, None], 0.)
        Rx = _np(got[0]).astype(np.float64)
        for b in range(shape[0]):
            assert np.abs(Rx[b] - want[b]).max() <= 2. ** -ref['sh'][b] + R.EPS[dtype] * want[b].max()
        assert ref['C'] == 1
        # the planes of an axis that is off, and its row vectors, are not looked at
        assert same(got, S.reassign_cwt_gpu(W, None, None, rsc, cst, None, None, gamma, return_acc=True))


# ------------------------------------------------------------------------------------------ order independence
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('idx', [TILE_PLUS_1, SCATTERED], ids=['tile_plus_1', 'scattered'])
def test_window_home_and_repeat_give_the_same_bits(S, idx, dtype):
    """A second launch, the launch that sends every term through a global atomic, and any `home` -- all zeros, reversed,
    scattered, out of range on either side -- are `torch.equal`: `home` and the window decide the speed only."""
    shape = shape_of(idx)
    rows = shape[1]
    for kind, flipud in (('log', True), ('linear', False)):
        a = run_case(S, shape, dtype, kind, flipud)
        Q.check('reassign_cwt_home_%d_%s' % (idx, dtype), a, reference(shape, dtype, kind, flipud), dtype)
        i32 = np.iinfo(np.int32)
        homes = [np.zeros(rows, dtype=int), np.arange(rows)[::-1], scattered_home(rows), np.full(rows, i32.max),
                 np.full(rows, i32.min), np.full(rows, -3), np.full(rows, rows + 2), np.arange(rows) * (1 << 40)]
        assert same(a, run_case(S, shape, dtype, kind, flipud))
        assert same(a, run_case(S, shape, dtype, kind, flipud, window=False))
        for home in homes:
            assert same(a, run_case(S, shape, dtype, kind, flipud, home=home)), home[:3]


@pytest.mark.parametrize('dtype', DTYPES)
def test_reversed_columns_give_the_same_bits(S, dtype):
    """The planes with their columns reversed and the group delays negated are the same scatter walked the other way
    round: the result is the reversed result, bit for bit."""
    import torch
    shape = shape_of(TILE_PLUS_1)
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
    freqs = Q.C.ssq_freqs('log', shape[1])
    a = run(S, W, dW, Wd, cst, rsc, dmax, freqs, gamma)
    b = run(S, W[..., ::-1], dW[..., ::-1], -Wd[..., ::-1], cst, rsc, dmax, freqs, gamma)
    assert torch.equal(a[0].flip(-1), b[0]) and torch.equal(a[1].flip(-1), b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_and_conservation(S, dtype):
    """A batch is its single calls; `acc` sums to the `q` of the points that land, as integers."""
    import torch
    shape = shape_of(BATCH)
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
    freqs = Q.C.ssq_freqs('log-piecewise', shape[1])
    Wv, Dv, Tv = dev(W), dev(dW), dev(Wd)
    Rx, acc, peak = run(S, Wv, Dv, Tv, cst, rsc, dmax, freqs, gamma, flipud=True)
    ref = reference(shape, dtype, 'log-piecewise', True)
    Q.check('reassign_cwt_batch_%s' % dtype, (Rx, acc, peak), ref, dtype)
    a = _np(acc).view(np.uint64)
    for b in range(shape[0]):
        one = run(S, Wv[b], Dv[b], Tv[b], cst, rsc, dmax, freqs, gamma, flipud=True)
        assert one[0].shape == Rx.shape[1:]
        assert torch.equal(one[0], Rx[b]) and torch.equal(one[1], acc[b]) and torch.equal(one[2], peak[b:b + 1]), b
        assert sum(map(int, a[b].reshape(-1))) == sum(map(int, ref['q'][b][ref['lands'][b]]))


# ------------------------------------------------------------------------------------------ crafted planes
def crafted_run(S, amp, k, d, freqs, cst, rsc, dmax, dtype, gamma=0., flipud=False, freq=True, time=True):
    W, dW, Wd = Q.crafted(amp, k, d, freqs, rsc, dtype)
    dW, Wd = dW if freq else None, Wd if time else None
    ref = Q.statement(W, dW, Wd, cst, rsc, dmax, freqs, gamma, flipud)
    assert ref['near_boundary'] == 0
    got = S.reassign_cwt_gpu(W, dW, Wd, rsc, cst, dmax, freqs, gamma, flipud=flipud, return_acc=True)
    Q.check('reassign_cwt_crafted', got, ref, dtype)
    return _np(got[0]).astype(np.float64), _np(got[1]).view(np.uint64), ref


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', GRIDS)
def test_rows_sent_to_given_bins_and_shifts(S, kind, dtype):
    """Every point of row `i` goes to bin ``kt[i]`` and moves by ``dt[i]`` columns: the closed form, on every grid and
    with `flipud`; two rows share a bin; targets off either end of the row are dropped."""
    rng = np.random.default_rng(5)
    rows, n = 7, 300
    freqs = Q.C.ssq_freqs(kind, rows)
    kt = np.array([3, 0, 6, 3, 1, 5, 2])
    dt = np.array([0, 2, -37, 11, -1, 40, 5])
    dmax = np.array([0, 2, 37, 12, 4, 40, 9], dtype=np.int32)
    rsc = np.array([1., 1.5, 3., 7., 8., 11.25, 64.])
    cst = rng.uniform(.5, 2., rows)
    amp = 1. + rng.random((1, rows, n))
    e = amp.astype(dtype).astype(np.float64) ** 2 * cst[None, :, None]
    for flipud in (False, True):
        Rx, acc, ref = crafted_run(S, amp, kt[None, :, None], dt[None, :, None], freqs, cst, rsc, dmax, dtype, flipud=flipud)
        want = np.zeros((1, rows, n))
        for i in range(rows):
            k = rows - 1 - kt[i] if flipud else kt[i]
            src = np.arange(n)
            ok = (src + dt[i] >= 0) & (src + dt[i] < n)
            want[0, k, src[ok] + dt[i]] += e[0, i, src[ok]]
        assert np.array_equal(Rx != 0, want != 0)
        # a term loses less than 2^-sh to the truncation (two terms meet in a cell at most), and the cell is rounded once
        assert np.abs(Rx - want).max() <= 2 * 2. ** -ref['sh'][0] + R.EPS[dtype] * want.max()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', GRIDS)
def test_frequencies_off_the_grid_land_in_the_end_bins(S, kind, dtype):
    """`w` below the grid lands in bin 0 and `w` above it in the top bin (the other way round with `flipud`), as
    `ssq_indexed_sum` clamps them; `w = 0` lands in bin 0."""
    rows, n = 6, 40
    freqs = Q.C.ssq_freqs(kind, rows)
    f = np.empty((1, rows, n))
    f[0, ::2], f[0, 1::2] = Q.C.F_LO / 7., Q.C.F_HI * 7.
    f[0, 2, :5] = 0.
    cst, rsc, dmax = np.ones(rows), np.ones(rows), np.zeros(rows, dtype=np.int32)
    for flipud in (False, True):
        Rx, acc, ref = crafted_run(S, 1.5, f, 0, freqs, cst, rsc, dmax, dtype, flipud=flipud)
        lo, hi = (rows - 1, 0) if flipud else (0, rows - 1)
        assert ((ref['k2'][0, ::2] == lo).all() and (ref['k2'][0, 1::2] == hi).all())
        # three rows of 1.5^2 meet in either end bin of every column (w = 0 is below any grid)
        assert (Rx[0][[lo, hi]] == 6.75).all() and not Rx[0][1:-1].any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_displacement_bound_is_per_row(S, dtype):
    """``|d| = dmax[i]`` is kept and ``dmax[i] + 1`` is dropped, row by row, in both directions; a point whose target
    lies off either end of the row is dropped."""
    rows, n = 6, 90
    dmax = np.array([0, 1, 2, 7, 20, 33], dtype=np.int32)
    rsc = np.array([1., 2., 3., 5., 9., 17.])
    freqs = Q.C.ssq_freqs('log', rows)
    d = np.zeros((1, rows, n))
    amp = np.full((1, rows, n), 1e-3)                       # below gamma but for the points placed
    want = np.zeros((1, rows, n))
    for i in range(rows):
        for j, (c, s) in enumerate(((40, 1), (42, -1), (44, 1), (46, -1))):
            dd = s * (dmax[i] + (j >= 2))                   # the first two at the bound, the other two one past it
            amp[0, i, c], d[0, i, c] = 2., dd
            if j < 2:
                want[0, i, c + dd] += 4.
        amp[0, i, 1], d[0, i, 1] = 2., -min(2, dmax[i])      # past the left end where dmax allows the move
        amp[0, i, n - 1], d[0, i, n - 1] = 2., min(1, dmax[i])
        if dmax[i] == 0:
            want[0, i, 1] += 4.
            want[0, i, n - 1] += 4.
        if dmax[i] == 1:
            want[0, i, 0] += 4.
    Rx, acc, ref = crafted_run(S, amp, np.arange(rows)[None, :, None], d, freqs, 1., rsc, dmax, dtype, gamma=.5, freq=False)
    assert np.array_equal(Rx, want)
    assert ref['peak'][0] == np.float64(4.).view(np.uint64)


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_point_into_one_cell_pins_the_headroom(S, dtype):
    """Every point of the plane goes to one cell, every term equal to the peak, ``n = 2 dmax + 1`` in every row: the cell
    holds ``C q`` exactly, below 2^62 and above 2^60 -- one bit less of headroom would overflow, one more would waste it."""
    rows, dm = 9, 35
    n = 2 * dm + 1
    freqs = Q.C.ssq_freqs('log', rows)
    c = np.arange(n)[None, None, :]
    dmax, rsc = np.full(rows, dm, dtype=np.int32), np.linspace(2., 40., rows)
    for amp in (1., 1.5, 3e-9):
        Rx, acc, ref = crafted_run(S, amp, 4, dm - c + 0 * np.arange(rows)[None, :, None], freqs, 1., rsc, dmax, dtype)
        Cn = rows * n
        q = int(ref['q'].max())
        assert int(acc[0, 4, dm]) == Cn * q and np.count_nonzero(acc) == 1
        assert 2 ** 60 <= Cn * q < 2 ** 62
        assert ref['C'] == Cn == Q.cell_terms(dmax, n, True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_cell_that_a_float32_running_sum_would_lose(S, dtype):
    """One cell receives a term of 1 and 2049 terms of 2^-30 from two rows: a running float32 sum stays at 1, the
    fixed-point sum is ``1 + 2049 2^-30`` exactly (rounded once to the output's precision), from either end."""
    n, rows = 1025, 2
    freqs = Q.C.ssq_freqs('linear', rows)
    c = np.arange(n)[None, None, :]
    amp = np.where(c == 0, 1., 2. ** -15) * np.ones((1, rows, 1))
    amp[0, 1, 0] = 2. ** -15
    s = np.float32(1.)
    for _ in range(2049):
        s = np.float32(s + np.float32(2. ** -30))
    assert s == 1.
    dmax, rsc = np.full(rows, n - 1, dtype=np.int32), np.array([1., 3.])
    for target, a in ((0, amp), (n - 1, amp[..., ::-1])):
        Rx, acc, ref = crafted_run(S, a, 1, target - c + 0 * amp, freqs, 1., rsc, dmax, dtype)
        assert Rx[0, 1, target] == np.float64(1. + 2049 * 2. ** -30).astype(dtype) > 1. and np.count_nonzero(Rx) == 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_points_below_gamma_and_non_finite_points(S, dtype):
    """Points below `gamma`, a NaN and an Inf point contribute nothing and do not set the peak; an all-zero signal in a
    batch gives zeros and leaves its neighbours alone."""
    rows, n = 4, 70
    rng = np.random.default_rng(9)
    freqs = Q.C.ssq_freqs('log', rows)
    amp = 1. + rng.random((3, rows, n))
    amp[1] = 0.
    amp[0, 1, 5], amp[0, 2, 6], amp[0, 3, 7] = np.nan, np.inf, 100.       # (100 is kept: the peak of signal 0)
    amp[2, 0, :10] = 1e-3
    k = rng.integers(0, rows, (3, rows, n))
    d = rng.integers(-3, 4, (3, rows, n))
    dmax, rsc, cst = np.full(rows, 3, dtype=np.int32), np.array([2., 3., 5., 9.]), np.array([1., .5, 2., .25])
    with np.errstate(all='ignore'):
        Rx, acc, ref = crafted_run(S, amp, k, d, freqs, cst, rsc, dmax, dtype, gamma=.5)
    assert ref['peak'][0] == np.float64(1e4 * .25).view(np.uint64) and ref['peak'][1] == 0
    assert not Rx[1].any() and Rx[0].any() and Rx[2].any() and np.isfinite(Rx).all()


# ------------------------------------------------------------------------------------------ links to the siblings
def test_freq_mode_is_indexed_sum_of_the_energy(S):
    """With the time axis off, float64: `Rx` is ``indexed_sum_onfly(|W|^2 + 0j, phase_cwt_gpu(W, dW, gamma), ...)`` to
    within the truncation of the cell's terms, ``rows 2^-sh`` at most, plus the running float64 sum's own rounding,
    ``rows eps`` of the cell."""
    import torch
    shape = shape_of(BATCH)
    rows = shape[1]
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, 'float64')
    for kind, flipud in (('log', True), ('log-piecewise', False), ('linear', True)):
        freqs = Q.C.ssq_freqs(kind, rows)
        ref = reference(shape, 'float64', kind, flipud, True, False)
        Rx = _np(run_case(S, shape, 'float64', kind, flipud, True, False)[0])
        Wv, Dv = dev(W), dev(dW)
        E = (Wv.real ** 2 + Wv.imag ** 2).to(torch.complex128)
        Tx = _np(S.indexed_sum_onfly(E, S.phase_cwt_gpu(Wv, Dv, gamma), freqs, cst, kind != 'linear', flipud)).real
        for b in range(shape[0]):
            tol = rows * 2. ** -ref['sh'][b] + (rows + 1) * R.EPS['float64'] * Rx[b]
            assert (np.abs(Tx[b] - Rx[b]) <= tol).all(), float(np.abs(Tx[b] - Rx[b]).max())


@pytest.mark.parametrize('dtype', DTYPES)
def test_time_mode_is_the_stft_form_row_by_row(S, dtype):
    """With the frequency axis off and ``cst = 1``, row `i` is `reassign2d_gpu`'s ``'time'`` form on the one-row plane
    with ``cols_per_second = rsc[i]`` and the same `dmax`, bit for bit in `acc` (``Re(-1j Wd / W) = Im(Wd / W)``, the
    same products in the same order). One `dmax` for all rows and one peak per row -- a point of magnitude 8 in every
    row -- so that both forms take the same shift."""
    rng = np.random.default_rng(21)
    rows, n, dm = 6, 300, 15
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    W = (rng.standard_normal((1, rows, n)) + 1j * rng.standard_normal((1, rows, n))).astype(cdt)
    W[0, :, 7] = 8.
    rsc = np.array([1., 2.5, 6., 11., 30., 64.])
    z = rng.standard_normal((1, rows, n)) + 1j * rng.standard_normal((1, rows, n))
    Wd = (W * (z * (.75 * dm / rsc)[None, :, None])).astype(cdt)
    dmax = np.full(rows, dm, dtype=np.int32)
    gamma = R.quiet_gamma(W)
    Rx, acc, peak = S.reassign_cwt_gpu(W, None, Wd, rsc, 1., dmax, None, gamma, return_acc=True)
    lands = Q.terms(W, None, Wd, np.ones(rows), rsc, dmax, None, gamma)[0]
    assert 0 < lands.mean() < 1
    for i in range(rows):
        one = S.reassign2d_gpu(W[:, i:i + 1], None, -1j * Wd[:, i:i + 1], 2, 1, rsc[i], gamma, dmax=dm, return_acc=True)
        assert np.array_equal(_np(one[1])[0, 0], _np(acc)[0, i]) and np.array_equal(_np(one[2]), _np(peak)), i
        assert np.array_equal(_np(one[0])[0, 0], _np(Rx)[0, i])


# ------------------------------------------------------------------------------------------ layouts and refusals
@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """`out=`, strided and lazily conjugated views, NumPy planes and tensor row vectors give the bits of the plain planes;
    so do pointers that are only 8-byte aligned, through the entry itself (the element-load instance in both dtypes)."""
    import torch
    from ssqueezepy_amd import _lib, algos
    shape = shape_of(BATCH)
    B, rows, n, top = shape
    W, dW, Wd, cst, rsc, dmax, gamma = case(shape, dtype)
    freqs = Q.C.ssq_freqs('log-piecewise', rows)
    Wv, Dv, Tv = dev(W), dev(dW), dev(Wd)
    args = (cst, rsc, dmax, freqs, gamma)
    want, want_acc, _ = run(S, Wv, Dv, Tv, *args, flipud=True)
    big = torch.zeros((B, rows, n + 3), dtype=Wv.dtype, device=DEV)
    big[..., 1:-2] = Wv
    conj = dev(np.conj(Wd)).conj()
    assert conj.is_conj() and not big[..., 1:-2].is_contiguous()
    assert torch.equal(run(S, big[..., 1:-2], Dv, conj, *args, flipud=True)[0], want)
    assert torch.equal(run(S, W, dW, Wd, *args, flipud=True)[0], want)          # NumPy planes
    assert torch.equal(run(S, Wv, Dv, Tv, torch.as_tensor(cst), torch.as_tensor(rsc), torch.as_tensor(dmax),
                           torch.as_tensor(freqs), gamma, flipud=True)[0], want)
    out = torch.full_like(want, -7.)
    assert run(S, Wv, Dv, Tv, *args, flipud=True, out=out)[0] is out and torch.equal(out, want)
    with pytest.raises(ValueError, match='`out`'):
        run(S, Wv, Dv, Tv, *args, out=out[..., ::2])
    with pytest.raises(ValueError, match='`out`'):
        run(S, Wv, Dv, Tv, *args, out=torch.zeros_like(Wv))
    with pytest.raises(ValueError, match='share one shape'):
        run(S, Wv, Dv[..., :-1], Tv, *args)
    with pytest.raises(TypeError):
        run(S, Wv.real, Dv, Tv, *args)
    for bad in (dict(cst=cst[:-1]), dict(rsc=rsc[:-1]), dict(dmax=dmax[:-1]), dict(freqs=freqs[:-1]),
                dict(home=np.zeros(rows + 1))):
        a = dict(cst=cst, rsc=rsc, dmax=dmax, freqs=freqs, home=None)
        a.update(bad)
        with pytest.raises(ValueError, match='one entry per row'):
            run(S, Wv, Dv, Tv, a['cst'], a['rsc'], a['dmax'], a['freqs'], gamma, home=a['home'])
    with pytest.raises(ValueError, match='`cst`'):
        run(S, Wv, Dv, Tv, -cst, rsc, dmax, freqs, gamma)
    with pytest.raises(ValueError, match='`gamma`'):
        run(S, Wv, Dv, Tv, cst, rsc, dmax, freqs, None)
    with pytest.raises(_lib.SsqError, match='ssq_reassign_cwt: dmax'):
        run(S, Wv, Dv, Tv, cst, rsc, -dmax - 1, freqs, gamma)

    # every plane 8 bytes past a 16-byte boundary: real buffers, the planes from their second element on
    lib = _lib.load()
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    step = 8 // (4 if dtype == 'float32' else 8)                           # reals in 8 bytes
    bufs = []
    for src in (Wv, Dv, Tv):
        buf = torch.zeros(2 * src.numel() + step, dtype=rdt, device=DEV)
        buf[step:] = torch.view_as_real(src).reshape(-1)
        assert buf.data_ptr() % 16 == 0
        bufs.append(buf)
    Rx = torch.full((B, rows, n), -7., dtype=rdt, device=DEV)
    acc = torch.zeros((B, rows, n), dtype=torch.int64, device=DEV)
    peak = torch.zeros((B,), dtype=torch.int64, device=DEV)
    cd, rd = dev(cst), dev(rsc)
    hd = dev(algos.reassign_cwt_home(rsc, freqs, True))
    kind, p = algos._grid(freqs, True)
    rc = lib.ssq_reassign_cwt(_lib.F32 if dtype == 'float32' else _lib.F64, bufs[0].data_ptr() + 8, bufs[1].data_ptr() + 8,
                              bufs[2].data_ptr() + 8, cd.data_ptr(), rd.data_ptr(), dmax.ctypes.data, hd.data_ptr(),
                              Rx.data_ptr(), acc.data_ptr(), peak.data_ptr(), B, rows, n, float(gamma), kind, p, 1,
                              _lib.REASSIGN_CWT_FREQ | _lib.REASSIGN_CWT_TIME, algos.stream())
    assert rc == 0, lib.ssq_last_error()
    sync()
    assert torch.equal(Rx, want) and torch.equal(acc, want_acc)


def test_abi_refusals_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib, algos
    lib = _lib.load()
    assert lib.ssq_version() >= 117 and _lib.ABI_VERSION >= 117 and 'ssq_reassign_cwt' in _lib.EXPORTS
    tr, tc, hr, hc, gcap, wr, wc = tile()
    assert tr >= 1 and tc >= 64 and hr >= 0 and hc >= 0 and gcap >= 1 and wr >= tr and wc == tc + 2 * hc
    assert lib.ssq_reassign_cwt_tile(7) == 0 and wr * wc * 8 <= 160 * 1024
    max_dmax = lib.ssq_time_reassign_max_dmax()
    assert max_dmax == Q.MAX_DMAX == algos.TSSQ_MAX_DMAX
    shape = (1, 5, 11, 4)
    B, rows, n, _ = shape
    W, dW, Wd, cst, rsc, dmax = Q.planes(shape, 'float64')
    freqs = Q.C.ssq_freqs('log', rows)
    kind, p = algos._grid(freqs, True)
    Wv, Dv, Tv, cd, rd, hd = dev(W), dev(dW), dev(Wd), dev(cst), dev(rsc), dev(np.arange(rows, dtype=np.int32))
    Rx = torch.full((B, rows, n), -7., dtype=torch.float64, device=DEV)
    acc = torch.full((B, rows, n), -7, dtype=torch.int64, device=DEV)
    peak = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    both = _lib.REASSIGN_CWT_FREQ | _lib.REASSIGN_CWT_TIME
    good = dict(W=Wv.data_ptr(), dW=Dv.data_ptr(), Wd=Tv.data_ptr(), cst=cd.data_ptr(), rsc=rd.data_ptr(), dmax=dmax,
                home=hd.data_ptr(), Rx=Rx.data_ptr(), acc=acc.data_ptr(), peak=peak.data_ptr(), batch=B, rows=rows, n=n,
                gamma=.5, grid=kind, params=p, flipud=0, flags=both)

    def call(**kw):
        a = dict(good, **kw)
        dm = a['dmax'].ctypes.data if a['dmax'] is not None else None
        return lib.ssq_reassign_cwt(_lib.F64, a['W'], a['dW'], a['Wd'], a['cst'], a['rsc'], dm, a['home'], a['Rx'],
                                    a['acc'], a['peak'], a['batch'], a['rows'], a['n'], a['gamma'], a['grid'], a['params'],
                                    a['flipud'], a['flags'], None)

    def with_dmax(i, v):
        dm = dmax.copy()
        dm[i] = v
        return dict(dmax=dm)
    nan = float('nan')
    refused = [dict(W=None), dict(dW=None), dict(Wd=None), dict(cst=None), dict(rsc=None), dict(dmax=None), dict(home=None),
               dict(Rx=None), dict(acc=None), dict(peak=None), dict(params=None), dict(batch=0), dict(rows=1), dict(rows=0),
               dict(n=0), dict(batch=1 << 20, rows=64, n=64), dict(gamma=-1.), dict(gamma=nan), dict(grid=3), dict(grid=-1),
               dict(flags=8), dict(flags=both | 16), with_dmax(0, -1), with_dmax(rows - 1, max_dmax + 1)]
    # (C >= 2^40 cannot be reached: C is at most rows * n, which the point count keeps below 2^32)
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_reassign_cwt'), (kw, lib.ssq_last_error())
        assert bool((Rx == -7.).all()) and bool((acc == -7).all()) and bool((peak == -7).all()), kw
    assert call() == 0
    # what an axis that is off does not need may be null; the window's `home` may be with the window off
    assert call(dW=None, params=None, grid=7, flags=_lib.REASSIGN_CWT_TIME) == 0
    assert call(Wd=None, rsc=None, dmax=None, flags=_lib.REASSIGN_CWT_FREQ) == 0
    assert call(home=None, flags=both | _lib.REASSIGN_CWT_NO_WINDOW) == 0 and call(**with_dmax(2, max_dmax)) == 0
    sync()
    assert not bool((Rx == -7.).any()) and not bool((acc == -7).any())


# ------------------------------------------------------------------------------------------ end to end
def signal(N):
    t = np.arange(N)
    rng = np.random.default_rng(11)
    return np.cos(2 * np.pi * (.11 * t + 1e-4 * t * t)) + (np.abs(t - N // 2) < 3) * 4. + .1 * rng.standard_normal(N)


@pytest.mark.parametrize('dtype', DTYPES)
def test_reassign_cwt_is_its_parts(S, dtype, N=1024):
    """`Wx` is `ssq_cwt`'s, `Rx` is `reassign_cwt_gpu` on separately executed plans; a batch is its single calls;
    `get_maps`; ``astensor=False``; the three modes; ``reassign='freq'`` makes one plan execution."""
    import torch
    from ssqueezepy_amd import Wavelet, algos, _cwt, wavelet_time_std
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    from ssqueezepy_amd.wavelets import derived_wavelets
    fs, nv = 50., 8
    wav = Wavelet(('gmw', {'dtype': dtype}), N=N)
    x = np.stack([signal(N), 1e2 * signal(N)[::-1].copy()])
    kw = dict(wavelet=wav, fs=fs, nv=nv)
    Rx, Wx, freqs, scales = S.reassign_cwt(x, **kw)
    sc_dt, grid_freqs, const, _, _ = _ssq_design(wav, 'log-piecewise', nv, N, 1 / fs, None, 'peak', True)
    na = len(scales)
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    assert Rx.shape == Wx.shape == (2, na, N) and Rx.dtype == rdt and not Rx.requires_grad
    assert np.array_equal(freqs, grid_freqs[::-1]) and np.array_equal(scales, sc_dt.squeeze())
    assert torch.equal(Wx, S.ssq_cwt(x, wav, fs=fs, nv=nv)[1])
    xd = torch.as_tensor(x.astype(dtype)).to(DEV)
    plan = _cwt.get_cwt_plan(wav, sc_dt, N, 'reflect', 1 / fs, True, 2)
    out = plan.execute(xd, want_dWx=True)
    Wd = _cwt.get_cwt_plan(derived_wavelets(wav)[0], sc_dt, N, 'reflect', 1 / fs, True, 2).execute(xd)['Wx']
    sc = np.asarray(sc_dt, dtype=np.float64).reshape(-1)
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wav), 4.)
    gamma = 10 * R.EPS[dtype]
    assert torch.equal(Wx, out['Wx'])
    assert torch.equal(Rx, S.reassign_cwt_gpu(out['Wx'], out['dWx'], Wd, sc, const, dmax, grid_freqs, gamma, flipud=True))
    Rf = S.reassign_cwt(x, reassign='freq', **kw)[0]
    Rt, Wt = S.reassign_cwt(x, reassign='time', **kw)[:2]
    assert torch.equal(Wt, Wx)
    assert torch.equal(Rf, S.reassign_cwt_gpu(out['Wx'], out['dWx'], None, sc, const, None, grid_freqs, gamma, flipud=True))
    assert torch.equal(Rt, S.reassign_cwt_gpu(out['Wx'], None, Wd, sc, const, dmax, None, gamma))
    assert not torch.equal(Rf, Rx) and not torch.equal(Rt, Rx)
    assert not torch.equal(Rx, S.reassign_cwt(x, max_shift=1., **kw)[0])
    assert torch.equal(Rx.flip(-2), S.reassign_cwt(x, flipud=False, **kw)[0])
    for b in range(2):
        one = S.reassign_cwt(x[b], **kw)
        assert torch.equal(one[0], Rx[b]) and torch.equal(one[1], Wx[b])
    xt = torch.as_tensor(x[0]).to(DEV).requires_grad_(True)
    Rg, Wg, _, _, f_hat, t_hat = S.reassign_cwt(xt, get_maps=True, **kw)
    assert all(a.grad_fn is None for a in (Rg, Wg, f_hat, t_hat)) and torch.equal(Rg, Rx[0])
    assert f_hat.shape == t_hat.shape == Wx[0].shape and f_hat.dtype == t_hat.dtype == rdt
    w0, d0, t0 = (_np(a[0]).astype(np.complex128) for a in (out['Wx'], out['dWx'], Wd))
    fh, th = _np(f_hat).astype(np.float64), _np(t_hat).astype(np.float64)
    low, kept = np.abs(w0) < .5 * gamma, np.abs(w0) >= 2 * gamma
    assert np.isinf(fh[low]).all() and np.isinf(th[low]).all()
    times = np.broadcast_to(np.arange(N) / fs, w0.shape)
    r = np.broadcast_to((sc / fs)[:, None], w0.shape)
    want_f = np.abs((d0[kept] / w0[kept]).imag) / (2 * np.pi)
    want_t = times[kept] + (-1j * r[kept] * t0[kept] / w0[kept]).real
    assert (np.abs(fh[kept] - want_f) <= 8 * R.EPS[dtype] * np.abs(d0[kept] / w0[kept])).all()
    assert (np.abs(th[kept] - want_t) <= 8 * R.EPS[dtype] * (np.abs(r[kept] * t0[kept] / w0[kept]) + times.max())).all()
    one = S.reassign_cwt(x[0], reassign='freq', get_maps=True, **kw)
    assert one[5] is None and one[4] is not None
    one = S.reassign_cwt(x[0], reassign='time', get_maps=True, **kw)
    assert one[4] is None and one[5] is not None
    outs = S.reassign_cwt(x[0], astensor=False, get_maps=True, **kw)
    assert all(isinstance(a, np.ndarray) for a in outs)
    assert np.array_equal(outs[0], _np(Rx[0])) and np.array_equal(outs[1], _np(Wx[0]))
    with pytest.raises(ValueError, match='`reassign`'):
        S.reassign_cwt(x[0], reassign='neither', **kw)
    with pytest.raises(NotImplementedError):
        S.reassign_cwt(x[0], wavelet='bump', fs=fs, nv=nv)
    with pytest.raises(NotImplementedError):
        S.reassign_cwt(x[0], wavelet=('gmw', {'order': 1}), fs=fs, nv=nv)

    # plan executions: two, but one for 'freq' -- and the `w psih` bank is never built
    calls = []
    execute = _cwt.CwtPlan.execute

    def counted(self, *a, **k):
        calls.append(k)
        return execute(self, *a, **k)
    _cwt.CwtPlan.execute = counted
    try:
        for mode, want in (('freq', [dict(want_dWx=True)]), ('time', [dict(want_dWx=False), {}]),
                           ('both', [dict(want_dWx=True), {}])):
            del calls[:]
            S.reassign_cwt(x[0], reassign=mode, **kw)
            assert calls == want, (mode, calls)
    finally:
        _cwt.CwtPlan.execute = execute


def impulse_case(N):
    """A unit impulse in the middle, a Morlet wavelet (mu = 13.4) and the scales from 8 to N / 16 samples, 16 to the
    octave: the rows whose wavelets resolve (centre frequency below Nyquist) and fit the signal on either side of the
    impulse -- `dmax`, and the 5.3 scales over which a row falls to 1e-6 of its peak."""
    n0 = N // 2
    x = np.zeros(N)
    x[n0] = 1.
    scales = 2. ** (3 + np.arange(16 * int(np.log2(N // 128)) + 1) / 16.)
    return x, n0, scales


@pytest.mark.parametrize('dtype', DTYPES)
def test_unit_impulse(S, dtype, N=1024):
    """A unit impulse at `n0`: every kept point's `t_hat` is within one sample of `n0` (the kept points above 1e-6 of the
    row's peak), and the share of `Rx` in the columns ``n0 - 1 .. n0 + 1`` agrees
    with the NumPy float64 restatement's (1e-3 absolute in float32, 1e-9 in float64); both are above 0.99."""
    from ssqueezepy_amd import Wavelet, algos, wavelet_time_std
    x, n0, scales = impulse_case(N)
    wav = Wavelet(('morlet', {'mu': 13.4, 'dtype': dtype}), N=N)
    Rx, Wx, freqs, sc, f_hat, t_hat = S.reassign_cwt(x, wav, scales=scales.astype(dtype), fs=1., get_maps=True)
    sc = np.asarray(sc, dtype=np.float64)
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wav), 4.)
    assert dmax.max() <= min(n0, N - 1 - n0)                            # every row's dmax fits the signal
    mag, th = np.abs(_np(Wx)).astype(np.float64), _np(t_hat).astype(np.float64)
    strong = (mag >= 2 * 10 * R.EPS[dtype]) & (mag > 1e-6 * mag.max(axis=1, keepdims=True))
    assert strong.any(axis=1).all() and np.isfinite(th[strong]).all()        # every row takes part
    print('impulse %s: largest |t_hat - n0| %.4f over %d points' % (dtype, np.abs(th[strong] - n0).max(), strong.sum()))
    assert np.abs(th[strong] - n0).max() <= 1.
    E = _np(Rx).astype(np.float64)
    share = float(E[:, n0 - 1:n0 + 2].sum() / E.sum())
    # the restatement, through the same design
    wav64 = Wavelet(('morlet', {'mu': 13.4, 'dtype': 'float64'}), N=N)
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    _, grid_freqs, const, _, _ = _ssq_design(wav, scales.astype(dtype), None, N, 1., None, 'peak', True)
    const = np.broadcast_to(np.asarray(const, dtype=np.float64).reshape(-1), sc.shape)
    W, dW, Wd = Q.np_planes(x, wav64, sc)
    A = Q.np_reassign(W, dW, Wd, sc, np.asarray(grid_freqs, dtype=np.float64), const, dmax, 10 * R.EPS['float64'])
    want = float(A[:, n0 - 1:n0 + 2].sum() / A.sum())
    print('impulse %s: share %.12f restatement %.12f' % (dtype, share, want))
    report_measured('reassign_cwt_impulse_%s' % dtype, share=share, restatement=want)
    assert abs(share - want) <= (1e-3 if dtype == 'float32' else 1e-9)
    assert share > .99 and want > .99


FM_PERIOD = 300.


@pytest.mark.parametrize('dtype', DTYPES)
def test_fm_tone_shares_are_ordered(S, dtype):
    """A frequency-modulated tone, ``0.15 + 0.05 cos(2 pi t / 300)`` cycles per sample, N = 4096, Morlet wavelet of mu =
    13.4, 32 voices: the share of the energy within +-1 row of the true frequency is in strict order, scalogram <
    min('freq', 'time') and max('freq', 'time') < 'both', and each is within 2e-3 of the NumPy float64 restatement's
    through the same design: 0.3440 / 0.6472 / 0.5865 / 0.9579. The bin-indexed planes ('freq', 'both') are read against
    the true bin of `ssq_freqs`, the row-indexed ones (the scalogram, 'time') against the rows' own centre frequencies
    (`reassign_cwt.row_freqs`)."""
    from ssqueezepy_amd import Wavelet
    x, f = Q.fm_tone(4096, FM_PERIOD)
    wav = Wavelet(('morlet', {'mu': 13.4, 'dtype': dtype}), N=4096)
    planes = {}
    for mode in ('freq', 'time', 'both'):
        Rx, Wx, freqs, sc = S.reassign_cwt(x, wav, nv=32, fs=1., reassign=mode)
        planes[mode] = _np(Rx).astype(np.float64)
    _, _, _, const, _ = Q.design(('morlet', {'mu': 13.4}), 4096)
    scal = np.abs(_np(Wx)).astype(np.float64) ** 2 * const[:, None]
    got = Q.fm_shares([scal, planes['freq'], planes['time'], planes['both']], f, np.asarray(freqs, dtype=np.float64),
                      Q.row_freqs(wav, sc))
    want = Q.np_fm_shares(FM_PERIOD)
    print('fm tone %s: scalogram %.4f freq %.4f time %.4f both %.4f; restatement %.4f %.4f %.4f %.4f' % (
        (dtype,) + tuple(got) + tuple(want)))
    report_measured('reassign_cwt_fm_tone_%s' % dtype, scalogram=got[0], freq=got[1], time=got[2], both=got[3])
    assert want[0] < min(want[1], want[2]) and max(want[1], want[2]) < want[3]
    assert got[0] < min(got[1], got[2]) and max(got[1], got[2]) < got[3]
    assert max(abs(g - w) for g, w in zip(got, want)) <= 2e-3
