# -*- coding: utf-8 -*-
"""`tssq_cwt`, `algos.time_reassign_cwt_gpu`, `algos.cwt_rotation_tables` and the entry `ssq_time_reassign_cwt` (the
time-reassigned synchrosqueezed CWT: a signed fixed-point scatter of rotated coefficients along their rows; DESIGN.md
section 4.5.12).

The oracle of the kernels is `tssq_cwt.statement`: the entry's definition in NumPy on separate real float64 arrays, one
ufunc per operation, the sum as `np.add.at` on int64, the rotation from the same two tables. `acc`, `peak` and `Tx` are
compared with `==` in both dtypes, and every seeded case asserts that the statement reports no point within 1e-6
(relative) of `gamma` -- nothing is left out of the comparison.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import reassign2d as R
import tssq_cwt as Q
from tssq_cwt import _np

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
SHAPE_IDS = Q.SHAPE_IDS
BATCH, TILE_PLUS_1, MIXED = SHAPE_IDS.index('batch'), SHAPE_IDS.index('tile_plus_1'), SHAPE_IDS.index('mixed_bounds')
# |share of the product - share of the restatement|, the larger of the two signals' values per dtype and signal length:
# N = 1024 measured on an MI355X, N = 512 under the emulator (profiles/tssq_cwt.txt); the tests assert four times it
SHARE_MEASURED = {('float32', 1024): 3.145e-08, ('float64', 1024): 2.220e-16,
                  ('float32', 512): 1.002e-06, ('float64', 512): 3.331e-16}


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def tile():
    """(tile rows, tile columns, halo columns, window columns, most workgroups, P) of the library in use."""
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    return tuple(lib.ssq_time_reassign_cwt_tile(i) for i in range(6))


def shape_of(idx):
    shapes = Q.shapes(*tile())
    assert len(shapes) == len(SHAPE_IDS)
    return shapes[idx]


_CASES, _REFS = {}, {}


def case(shape, dtype):
    """Planes, row vectors, host tables and a `gamma` midway between two neighbouring samples of ``|W|`` near the lower
    quartile of the smallest signal; made once, nobody writes to them."""
    key = (shape, dtype)
    if key not in _CASES:
        W, Wd, rsc, dmax, phi = Q.planes(shape, dtype, hc=tile()[2])
        _CASES[key] = (W, Wd, rsc, dmax, Q.tables(phi, shape[2]), R.quiet_gamma(W))
    return _CASES[key]


def reference(shape, dtype, rot=True):
    key = (shape, dtype, rot)
    if key not in _REFS:
        W, Wd, rsc, dmax, tab, gamma = case(shape, dtype)
        _REFS[key] = Q.statement(W, Wd, rsc, dmax, tab if rot else None, gamma)
    return _REFS[key]


def run(S, W, Wd, rsc, dmax, rot, gamma, **kw):
    return S.time_reassign_cwt_gpu(W, Wd, rsc, dmax, gamma, rot=rot, return_acc=True, **kw)


def run_case(S, shape, dtype, rot=True, **kw):
    W, Wd, rsc, dmax, tab, gamma = case(shape, dtype)
    return run(S, W, Wd, rsc, dmax, tab if rot else False, gamma, **kw)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def sync():
    import torch
    torch.cuda.synchronize() if DEV == 'cuda' else None


def same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def outside_window(ref, n):
    """Per point: whether its target column lies outside the LDS window of its tile."""
    tr, tc, hc, wc, gcap, p = tile()
    c = np.arange(n)[None, None, :]
    return (ref['c2'] < c // tc * tc - hc) | (ref['c2'] >= c // tc * tc - hc + wc)


# ------------------------------------------------------------------------------------------ kernels against statement
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('idx', range(len(SHAPE_IDS)), ids=SHAPE_IDS)
def test_kernel_vs_statement(S, idx, dtype):
    tr, tc, hc, wc, gcap, p = tile()
    assert p == Q.P == tc
    shape = shape_of(idx)
    B, rows, n, top = shape
    ref = reference(shape, dtype)
    assert ref['near_gamma'] == 0                           # the condition the equalities rest on
    lands = ref['lands']
    assert 0 < lands.mean() < 1                             # some points are dropped, some land
    if B > 1:
        assert len(set(ref['sh'])) == B                     # a shift per signal
    out = outside_window(ref, n) & lands
    outside = float(out.sum() / max(lands.sum(), 1))
    if SHAPE_IDS[idx] in Q.LEAVES:
        assert n > wc and case(shape, dtype)[3].max() >= 2 * hc
        assert out.any() and (lands & ~out).any()           # some terms leave the window, some stay
    if SHAPE_IDS[idx] == 'more_tiles_than_workgroups':
        assert B * -(-rows // tr) * -(-n // tc) > gcap
    if SHAPE_IDS[idx] == 'three_rot_hi':
        assert n % p and -(-n // p) == 3
    if idx == MIXED:
        assert case(shape, dtype)[3].tolist() == [0, hc - 1, hc, hc + 1, n + 50, 3]
    got = run_case(S, shape, dtype)
    Q.check('tssq_cwt_%s_%s' % (SHAPE_IDS[idx], dtype), got, ref, dtype)
    report_measured('tssq_cwt_kernel_%s_%s' % (SHAPE_IDS[idx], dtype), landed=float(lands.mean()),
                    outside_window=outside, filled=float((ref['acc'] != 0).any(axis=-1).mean()))


# ------------------------------------------------------------------------------------------ order and schedule
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('idx', [TILE_PLUS_1, MIXED], ids=['tile_plus_1', 'mixed_bounds'])
def test_window_and_repeat_give_the_same_bits(S, idx, dtype):
    """A second launch and the launch that sends every term through global atomics are `torch.equal`, with the tables and
    without them."""
    shape = shape_of(idx)
    for rot in (True, False):
        a = run_case(S, shape, dtype, rot)
        Q.check('tssq_cwt_repeat_%d_%s' % (idx, dtype), a, reference(shape, dtype, rot), dtype)
        assert same(a, run_case(S, shape, dtype, rot))
        assert same(a, run_case(S, shape, dtype, rot, window=False))


@pytest.mark.parametrize('dtype', DTYPES)
def test_reversed_columns_give_the_reversed_acc(S, dtype):
    """With the tables off, the planes with their columns reversed and the group delays negated are the same scatter
    walked the other way round: the reversed result, bit for bit."""
    import torch
    W, Wd, rsc, dmax, tab, gamma = case(shape_of(TILE_PLUS_1), dtype)
    a = run(S, W, Wd, rsc, dmax, False, gamma)
    b = run(S, W[..., ::-1], -Wd[..., ::-1], rsc, dmax, False, gamma)
    assert torch.equal(a[0].flip(-1), b[0]) and torch.equal(a[1].flip(-2), b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_and_conservation(S, dtype):
    """A batch is its single calls; per row and component `acc` sums to the `q` of the points that land, as integers."""
    import torch
    shape = shape_of(BATCH)
    W, Wd, rsc, dmax, tab, gamma = case(shape, dtype)
    Wv, Tv = dev(W), dev(Wd)
    Tx, acc, peak = run(S, Wv, Tv, rsc, dmax, tab, gamma)
    ref = reference(shape, dtype)
    Q.check('tssq_cwt_batch_%s' % dtype, (Tx, acc, peak), ref, dtype)
    a = _np(acc)
    for b in range(shape[0]):
        one = run(S, Wv[b], Tv[b], rsc, dmax, tab, gamma)
        assert one[0].shape == Tx.shape[1:] and one[1].shape == acc.shape[1:]
        assert torch.equal(one[0], Tx[b]) and torch.equal(one[1], acc[b]) and torch.equal(one[2], peak[b:b + 1]), b
        for i in range(shape[1]):
            for k in range(2):
                assert sum(map(int, a[b, i, :, k])) == sum(map(int, ref['q'][b, i, :, k])), (b, i, k)


# ------------------------------------------------------------------------------------------ crafted planes
def crafted_run(S, amp, d, rsc, dmax, dtype, gamma=0., rot=None):
    W, Wd = Q.crafted(amp, d, rsc, dtype)
    ref = Q.statement(W, Wd, rsc, dmax, rot, gamma)
    got = S.time_reassign_cwt_gpu(W, Wd, rsc, dmax, gamma, rot=False if rot is None else rot, return_acc=True)
    Q.check('tssq_cwt_crafted', got, ref, dtype)
    return _np(got[0]).astype(np.complex128), _np(got[1]), ref


@pytest.mark.parametrize('dtype', DTYPES)
def test_rows_sent_to_given_shifts(S, dtype):
    """Every point of row `i` moves by ``dt[i]`` columns: the closed form; targets off either edge of the plane are
    dropped."""
    rng = np.random.default_rng(5)
    rows, n = 7, 300
    dt = np.array([0, 2, -37, 11, -1, 40, 5])
    dmax = np.array([0, 2, 37, 12, 4, 40, 9], dtype=np.int32)
    rsc = np.array([1., 1.5, 3., 7., 8., 11.25, 64.])
    amp = (1. + rng.random((1, rows, n))) * np.exp(2j * np.pi * rng.random((1, rows, n)))
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    z = amp.astype(cdt).astype(np.complex128)
    Tx, acc, ref = crafted_run(S, amp, dt[None, :, None], rsc, dmax, dtype)
    want = np.zeros((1, rows, n), dtype=np.complex128)
    for i in range(rows):
        src = np.arange(n)
        ok = (src + dt[i] >= 0) & (src + dt[i] < n)
        want[0, i, src[ok] + dt[i]] = z[0, i, src[ok]]
        assert not ref['lands'][0, i, ~ok].any() and ref['lands'][0, i, ok].all()          # drops at both edges
    assert np.array_equal(Tx != 0, want != 0)
    # one term per cell: a component loses less than 2^-sh to the truncation, and the cell is rounded once
    for part in (np.real, np.imag):
        assert np.abs(part(Tx) - part(want)).max() <= 2. ** -ref['sh'][0] + R.EPS[dtype] * np.abs(want).max()


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_displacement_bound_is_per_row(S, dtype):
    """``|d| = dmax[i]`` is kept and ``dmax[i] + 1`` is dropped, row by row, in both directions."""
    rows, n = 6, 90
    dmax = np.array([0, 1, 2, 7, 20, 33], dtype=np.int32)
    rsc = np.array([1., 2., 3., 5., 9., 17.])
    d = np.zeros((1, rows, n))
    amp = np.full((1, rows, n), 1e-3)                       # below gamma but for the points placed
    want = np.zeros((1, rows, n))
    for i in range(rows):
        for j, (c, s) in enumerate(((40, 1), (42, -1), (44, 1), (46, -1))):
            dd = s * (dmax[i] + (j >= 2))                   # the first two at the bound, the other two one past it
            amp[0, i, c], d[0, i, c] = 2., dd
            if j < 2:
                want[0, i, c + dd] += 2.
    Tx, acc, ref = crafted_run(S, amp, d, rsc, dmax, dtype, gamma=.5)
    assert np.array_equal(Tx, want.astype(np.complex128))
    assert ref['peak'][0] == np.float64(4.).view(np.uint64)


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_window_edge_is_at_the_halo(S, dtype):
    """Shifts of exactly ``HC`` and ``HC + 1`` from the first and the last column of a tile, in both directions: ``-HC``
    from column 0 and ``+HC`` from column ``TC - 1`` land on the window's first and last cell, one further leaves it (the
    window is ``[c0 - HC, c0 + TC + HC)``), and either way the cell holds the term; so do the neighbours of each."""
    tr, tc, hc, wc, gcap, p = tile()
    rows, n = 2, 3 * tc + 2 * hc + 7
    ct = (hc + tc) // tc + 1                                 # a tile with hc + 1 columns of the plane on either side
    c0 = ct * tc
    assert c0 - hc - 1 >= 0 and c0 + tc - 1 + hc + 1 < n
    d = np.zeros((1, rows, n))
    amp = np.full((1, rows, n), 1e-3, dtype=np.complex128)   # below gamma but for the points placed
    want = np.zeros((1, rows, n), dtype=np.complex128)
    places = [(0, c0, -hc), (0, c0 + 1, -hc - 2), (0, c0 + tc - 1, hc), (0, c0 + tc - 2, hc + 2),
              (1, c0, -hc - 1), (1, c0 + 1, -hc - 1), (1, c0 + tc - 1, hc + 1), (1, c0 + tc - 2, hc + 1)]
    for k, (i, c, dd) in enumerate(places):
        amp[0, i, c], d[0, i, c] = (k + 2.) * (1 - 1j), dd
        want[0, i, c + dd] += amp[0, i, c]
    dmax, rsc = np.full(rows, hc + 2, dtype=np.int32), np.array([3., 7.])
    Tx, acc, ref = crafted_run(S, amp, d, rsc, dmax, dtype, gamma=.5)
    out = (outside_window(ref, n) & ref['lands'])[0]
    got = sorted((int(i), int(c)) for i, c in np.argwhere(out))
    # the shifts of hc stay; hc + 1 from an edge column and hc + 2 from the column next to it leave; hc + 1 from the
    # column next to the edge lands on the window's edge cell
    assert got == [(0, c0 + 1), (0, c0 + tc - 2), (1, c0), (1, c0 + tc - 1)], got
    assert np.array_equal(Tx, want) and int(ref['lands'].sum()) == len(places)


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_point_of_a_row_into_one_cell_pins_the_headroom(S, dtype):
    """Every point of a row goes to one cell, every term at the peak magnitude with one sign in both components, ``n = 2
    dmax + 1``: the cell holds ``n q`` exactly in both components, below 2^62 -- and, with ``n = 2^k - 1`` terms of
    magnitude ``sqrt(emax)`` just below a power of two, above 2^59: one bit less of headroom could overflow for an odd
    exponent, one more would waste it."""
    dm = 63
    n = 2 * dm + 1
    rows = 2
    c = np.arange(n)[None, None, :]
    dmax, rsc = np.full(rows, dm, dtype=np.int32), np.array([2., 40.])
    for re, im in ((1., 1.), (-1.5, -1.5), (3e-9, 3e-9), (.999, .999), (-.7, .7)):
        Tx, acc, ref = crafted_run(S, re + 1j * im, dm - c + 0 * np.arange(rows)[None, :, None], rsc, dmax, dtype)
        q = ref['q'][0, 0, 0]
        assert ref['C'] == n and (ref['q'][0] == q).all()
        for i in range(rows):
            assert [int(v) for v in acc[0, i, dm]] == [n * int(q[0]), n * int(q[1])]
        assert np.count_nonzero(acc) == 2 * rows and int(np.abs(acc).max()) < 2 ** 62
        assert int(np.abs(acc).max()) >= 2 ** 59
    assert (acc[0, :, dm, 0] < 0).all() and (acc[0, :, dm, 1] > 0).all()     # the last case: signed components
    assert (Tx[0, :, dm].real < 0).all() and (Tx[0, :, dm].imag > 0).all()  # ... which the finish reads as signed


@pytest.mark.parametrize('dtype', DTYPES)
def test_cancelling_pairs_leave_the_small_terms_exact(S, dtype):
    """One cell receives pairs of +-2^45 (1 + i) around terms of 1 - 2i: the sum is ``k (1 - 2i)`` exactly, where a float32
    (and a float64 running sum of such pairs in an unlucky order) would lose the small terms."""
    dm = 8
    n = 2 * dm + 1
    c = np.arange(n)[None, None, :]
    amp = np.empty((1, 1, n), dtype=np.complex128)
    amp[0, 0, 0::3], amp[0, 0, 1::3], amp[0, 0, 2::3] = 2. ** 45 * (1 + 1j), 1 - 2j, -2. ** 45 * (1 + 1j)
    amp[0, 0, 15:] = 1 - 2j                                   # (17 = 3 x 5 + 2: the unpaired tail is small terms)
    assert np.float32(np.float32(2. ** 45) + np.float32(1.)) == np.float32(2. ** 45)
    small = int((amp[0, 0] == 1 - 2j).sum())
    assert abs(amp.sum() - small * (1 - 2j)) == 0 and small == 7
    Tx, acc, ref = crafted_run(S, amp, dm - c, np.array([3.]), np.array([dm], dtype=np.int32), dtype)
    assert Tx[0, 0, dm] == small * (1 - 2j) and np.count_nonzero(Tx) == 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_rotation_alone_and_no_rotation(S, dtype):
    """``W = 1``, ``d = 0``: `acc` is the truncated product ``rot_hi rot_lo`` at every column, across two `P` boundaries,
    and `Tx` is the rotation to the fixed-point bound; with NULL tables the terms are `W` itself."""
    P = tile()[5]
    rows, n = 3, 2 * P + 9
    phi = np.array([.3137, .04321, 1. / 3.])
    tab = Q.tables(phi, n)
    rsc, dmax = np.ones(rows), np.zeros(rows, dtype=np.int32)
    Tx, acc, ref = crafted_run(S, 1., np.zeros((1, rows, n)), rsc, dmax, dtype, rot=tab)
    c = np.arange(n)
    u = tab[1][:, c // P] * 0
    u.real = tab[1].real[:, c // P] * tab[0].real[:, c % P] - tab[1].imag[:, c // P] * tab[0].imag[:, c % P]
    u.imag = tab[1].real[:, c // P] * tab[0].imag[:, c % P] + tab[1].imag[:, c // P] * tab[0].real[:, c % P]
    sh = ref['sh'][0]
    assert sh == 61 - 1 - 1                                   # emax = 1 = 0.5 x 2^1; C = 1
    assert np.array_equal(acc[0, ..., 0], np.trunc(np.ldexp(u.real, sh)).astype(np.int64))
    assert np.array_equal(acc[0, ..., 1], np.trunc(np.ldexp(u.imag, sh)).astype(np.int64))
    exact = np.exp(-2j * np.pi * np.mod(phi[:, None] * c[None, :], 1.))
    assert np.abs(Tx[0] - exact).max() <= 2. ** -sh + 2 * R.EPS[dtype] + n * R.EPS['float64']
    rng = np.random.default_rng(8)
    amp = rng.standard_normal((1, rows, n)) + 1j * rng.standard_normal((1, rows, n))
    Tx, acc, ref = crafted_run(S, amp, np.zeros((1, rows, n)), rsc, dmax, dtype)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    assert np.abs(Tx - amp.astype(cdt)).max() <= 2 * 2. ** -ref['sh'][0] + R.EPS[dtype] * np.abs(amp).max()


@pytest.mark.parametrize('dtype', DTYPES)
def test_points_below_gamma_and_non_finite_points(S, dtype):
    """Points below `gamma`, a NaN and an Inf point contribute nothing and do not set the peak; an all-zero signal in a
    batch gives zeros and leaves its neighbours alone; all-NaN and all-Inf planes give zeros."""
    rows, n = 4, 70
    rng = np.random.default_rng(9)
    amp = (1. + rng.random((3, rows, n))).astype(np.complex128)
    amp[1] = 0.
    amp[0, 1, 5], amp[0, 2, 6], amp[0, 3, 7] = np.nan, np.inf, 100.       # (100 is kept: the peak of signal 0)
    amp[2, 0, :10] = 1e-3
    d = rng.integers(-3, 4, (3, rows, n))
    dmax, rsc = np.full(rows, 3, dtype=np.int32), np.array([2., 3., 5., 9.])
    with np.errstate(all='ignore'):
        Tx, acc, ref = crafted_run(S, amp, d, rsc, dmax, dtype, gamma=.5)
        assert ref['peak'][0] == np.float64(1e4).view(np.uint64) and ref['peak'][1] == 0
        assert not Tx[1].any() and Tx[0].any() and Tx[2].any() and np.isfinite(Tx).all()
        for bad in (np.nan, np.inf):
            Tx, acc, ref = crafted_run(S, np.full((1, rows, n), bad), d[:1], rsc, dmax, dtype, gamma=.5)
            assert not Tx.any() and not acc.any() and ref['peak'][0] == 0


# ------------------------------------------------------------------------------------------ links to the siblings
@pytest.mark.parametrize('dtype', DTYPES)
def test_unit_magnitudes_count_terms_like_reassign_cwt(S, dtype):
    """With ``W = 1`` everywhere, the tables off and ``cst = 1``, ``ldexp(acc_re, -sh)`` equals `reassign_cwt_gpu`'s
    time-only `Rx`: both count a cell's terms, exactly; and the two statements take the same `d`."""
    import reassign_cwt as RC
    rng = np.random.default_rng(21)
    rows, n = 6, 300
    dmax = np.array([0, 3, 15, 15, 70, 200], dtype=np.int32)
    rsc = np.array([1., 2.5, 6., 11., 30., 64.])
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    W = np.ones((1, rows, n), dtype=cdt)
    z = rng.standard_normal((1, rows, n)) + 1j * rng.standard_normal((1, rows, n))
    Wd = (z * (.75 * np.maximum(dmax, 1) / rsc)[None, :, None]).astype(cdt)
    Tx, acc, peak = S.time_reassign_cwt_gpu(W, Wd, rsc, dmax, .5, rot=False, return_acc=True)
    ref = Q.statement(W, Wd, rsc, dmax, None, .5)
    Q.check('tssq_cwt_counts', (Tx, acc, peak), ref, dtype)
    sib = RC.terms(W, None, Wd, np.ones(rows), rsc, dmax, None, .5)
    assert np.array_equal(sib[0], ref['lands']) and np.array_equal(sib[2], ref['c2'])
    assert 0 < ref['lands'].mean() < 1
    Rx = _np(S.reassign_cwt_gpu(W, None, Wd, rsc, 1., dmax, None, .5)).astype(np.float64)
    counts = np.ldexp(_np(acc)[..., 0].astype(np.float64), -ref['sh'][0])
    assert np.array_equal(counts, Rx) and counts.max() > 1 and not _np(acc)[..., 1].any()
    assert counts.sum() == ref['lands'].sum()


# ------------------------------------------------------------------------------------------ layouts and refusals
@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """`out=`, strided and lazily conjugated views, NumPy planes and tensor row vectors give the bits of the plain planes;
    so do pointers that are only 8-byte aligned, through the entry itself (the element-load instance in both dtypes)."""
    import torch
    from ssqueezepy_amd import _lib, algos
    shape = shape_of(BATCH)
    B, rows, n, top = shape
    W, Wd, rsc, dmax, tab, gamma = case(shape, dtype)
    Wv, Tv = dev(W), dev(Wd)
    tabv = (dev(tab[0]), dev(tab[1]))
    want, want_acc, want_peak = run(S, Wv, Tv, rsc, dmax, tabv, gamma)
    Q.check('tssq_cwt_layouts_%s' % dtype, (want, want_acc, want_peak), reference(shape, dtype), dtype)
    big = torch.zeros((B, rows, n + 3), dtype=Wv.dtype, device=DEV)
    big[..., 1:-2] = Wv
    conj = dev(np.conj(Wd)).conj()
    assert conj.is_conj() and not big[..., 1:-2].is_contiguous()
    assert torch.equal(run(S, big[..., 1:-2], conj, rsc, dmax, tabv, gamma)[0], want)
    assert torch.equal(run(S, W, Wd, rsc, dmax, tab, gamma)[0], want)              # NumPy planes and tables
    assert torch.equal(run(S, Wv, Tv, torch.as_tensor(rsc), torch.as_tensor(dmax), tabv, gamma)[0], want)
    out = torch.full_like(want, -7.)
    assert run(S, Wv, Tv, rsc, dmax, tabv, gamma, out=out)[0] is out and torch.equal(out, want)
    # the Python refusals
    with pytest.raises(ValueError, match='`out`'):
        run(S, Wv, Tv, rsc, dmax, tabv, gamma, out=out[..., ::2])
    with pytest.raises(ValueError, match='`out`'):
        run(S, Wv, Tv, rsc, dmax, tabv, gamma, out=torch.zeros_like(Wv.real))
    with pytest.raises(ValueError, match='share one shape'):
        run(S, Wv, Tv[..., :-1], rsc, dmax, tabv, gamma)
    with pytest.raises(TypeError):
        run(S, Wv.real, Tv, rsc, dmax, tabv, gamma)
    with pytest.raises(ValueError, match='one entry per row'):
        run(S, Wv, Tv, rsc[:-1], dmax, tabv, gamma)
    with pytest.raises(ValueError, match='one entry per row'):
        run(S, Wv, Tv, rsc, dmax[:-1], tabv, gamma)
    with pytest.raises(ValueError, match='cwt_rotation_tables'):
        run(S, Wv, Tv, rsc, dmax, None, gamma)
    with pytest.raises(ValueError, match='`rot`'):
        run(S, Wv, Tv, rsc, dmax, (tabv[0], tabv[1][:, :-1]), gamma)
    with pytest.raises(ValueError, match='`rot`'):
        run(S, Wv, Tv, rsc, dmax, tabv[0], gamma)
    with pytest.raises(ValueError, match='`gamma`'):
        run(S, Wv, Tv, rsc, dmax, tabv, None)
    with pytest.raises(_lib.SsqError, match='ssq_time_reassign_cwt: dmax'):
        run(S, Wv, Tv, rsc, -dmax - 1, tabv, gamma)
    for bad in ([1., np.nan], [1., 0.], [-1., 1.], [np.inf, 1.]):
        with pytest.raises(ValueError, match='`row_freqs`'):
            S.cwt_rotation_tables(bad, 10)
    # `cwt_rotation_tables` is the host form on the device, cached per content
    phi = np.array([.25, .1234567])
    lo, hi = S.cwt_rotation_tables(phi * 50., 700, fs=50.)
    want_lo, want_hi = Q.tables(phi * 50. / 50., 700)
    assert lo.dtype == hi.dtype == torch.complex128 and lo.shape == (2, Q.P) and hi.shape == (2, 3)
    assert np.array_equal(_np(lo), want_lo) and np.array_equal(_np(hi), want_hi)
    assert S.cwt_rotation_tables(phi * 50., 700, fs=50.)[0] is lo

    # every plane 8 bytes past a 16-byte boundary: real buffers, the planes from their second element on
    lib = _lib.load()
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    step = 8 // (4 if dtype == 'float32' else 8)                           # reals in 8 bytes
    bufs = []
    for src in (Wv, Tv):
        buf = torch.zeros(2 * src.numel() + step, dtype=rdt, device=DEV)
        buf[step:] = torch.view_as_real(src).reshape(-1)
        assert buf.data_ptr() % 16 == 0
        bufs.append(buf)
    Txb = torch.full((2 * B * rows * n + step,), -7., dtype=rdt, device=DEV)
    acc = torch.zeros((B, rows, n, 2), dtype=torch.int64, device=DEV)
    peak = torch.zeros((B,), dtype=torch.int64, device=DEV)
    rd = dev(rsc)
    rc = lib.ssq_time_reassign_cwt(_lib.F32 if dtype == 'float32' else _lib.F64, bufs[0].data_ptr() + 8,
                                   bufs[1].data_ptr() + 8, rd.data_ptr(), dmax.ctypes.data, tabv[0].data_ptr(),
                                   tabv[1].data_ptr(), Txb.data_ptr() + 8, acc.data_ptr(), peak.data_ptr(), B, rows, n,
                                   float(gamma), 0, algos.stream())
    assert rc == 0, lib.ssq_last_error()
    sync()
    assert torch.equal(Txb[step:], torch.view_as_real(want).reshape(-1)) and torch.equal(acc, want_acc)
    assert bool((Txb[:step] == -7.).all())


def test_abi_refusals_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib, algos
    lib = _lib.load()
    assert lib.ssq_version() >= 120 and _lib.ABI_VERSION >= 120 and 'ssq_time_reassign_cwt' in _lib.EXPORTS
    tr, tc, hc, wc, gcap, p = tile()
    assert tr >= 1 and tc >= 64 and hc >= 0 and gcap >= 1 and wc == tc + 2 * hc and p == _lib.TSSQ_CWT_ROT_P == tc
    assert lib.ssq_time_reassign_cwt_tile(6) == 0 and tr * wc * 16 <= 160 * 1024
    max_dmax = lib.ssq_time_reassign_max_dmax()
    assert max_dmax == Q.MAX_DMAX == algos.TSSQ_MAX_DMAX
    shape = (1, 5, 11, 4)
    B, rows, n, _ = shape
    W, Wd, rsc, dmax, phi = Q.planes(shape, 'float64')
    tab = Q.tables(phi, n)
    Wv, Tv, rd, lo, hi = dev(W), dev(Wd), dev(rsc), dev(tab[0]), dev(tab[1])
    Tx = torch.full((B, rows, n), -7., dtype=torch.complex128, device=DEV)
    acc = torch.full((B, rows, n, 2), -7, dtype=torch.int64, device=DEV)
    peak = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    good = dict(W=Wv.data_ptr(), Wd=Tv.data_ptr(), rsc=rd.data_ptr(), dmax=dmax, lo=lo.data_ptr(), hi=hi.data_ptr(),
                Tx=Tx.data_ptr(), acc=acc.data_ptr(), peak=peak.data_ptr(), batch=B, rows=rows, n=n, gamma=.5, flags=0)

    def call(**kw):
        a = dict(good, **kw)
        dm = a['dmax'].ctypes.data if a['dmax'] is not None else None
        return lib.ssq_time_reassign_cwt(_lib.F64, a['W'], a['Wd'], a['rsc'], dm, a['lo'], a['hi'], a['Tx'], a['acc'],
                                         a['peak'], a['batch'], a['rows'], a['n'], a['gamma'], a['flags'], None)

    def with_dmax(i, v):
        dm = dmax.copy()
        dm[i] = v
        return dict(dmax=dm)
    nan = float('nan')
    refused = [dict(W=None), dict(Wd=None), dict(rsc=None), dict(dmax=None), dict(Tx=None), dict(acc=None), dict(peak=None),
               dict(lo=None), dict(hi=None), dict(batch=0), dict(rows=0), dict(n=0), dict(batch=1 << 19, rows=64, n=64),
               dict(batch=1, rows=1, n=1 << 31), dict(gamma=-1.), dict(gamma=nan), dict(flags=2), dict(flags=1 | 4),
               with_dmax(0, -1), with_dmax(rows - 1, max_dmax + 1)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_time_reassign_cwt'), (kw, lib.ssq_last_error())
        assert bool((Tx == -7.).all()) and bool((acc == -7).all()) and bool((peak == -7).all()), kw
    assert call() == 0
    assert call(lo=None, hi=None) == 0 and call(flags=_lib.TSSQ_CWT_NO_WINDOW) == 0 and call(**with_dmax(2, max_dmax)) == 0
    sync()
    assert not bool((Tx == -7.).any()) and not bool((acc == -7).any())


# ------------------------------------------------------------------------------------------ end to end
def signal(N):
    t = np.arange(N)
    rng = np.random.default_rng(11)
    return np.cos(2 * np.pi * (.11 * t + 1e-4 * t * t)) + (np.abs(t - N // 2) < 3) * 4. + .1 * rng.standard_normal(N)


@pytest.mark.parametrize('dtype', DTYPES)
def test_tssq_cwt_is_its_parts(S, dtype, N=1024):
    """`Wx` is `ssq_cwt`'s, `Tx` is `time_reassign_cwt_gpu` on separately executed plans; a batch is its single calls;
    `get_t`; ``astensor=False``; two plan executions, neither with `dWx`."""
    import torch
    from ssqueezepy_amd import Wavelet, algos, _cwt, wavelet_time_std, row_frequencies
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    from ssqueezepy_amd.wavelets import derived_wavelets
    fs, nv = 50., 8
    wav = Wavelet(('gmw', {'dtype': dtype}), N=N)
    x = np.stack([signal(N), 1e2 * signal(N)[::-1].copy()])
    kw = dict(wavelet=wav, fs=fs, nv=nv)
    Tx, Wx, freqs, scales = S.tssq_cwt(x, **kw)
    sc_dt = _ssq_design(wav, 'log-piecewise', nv, N, 1 / fs, None, 'peak', True)[0]
    na = len(scales)
    cdt = torch.complex64 if dtype == 'float32' else torch.complex128
    assert Tx.shape == Wx.shape == (2, na, N) and Tx.dtype == cdt and not Tx.requires_grad
    sc = np.asarray(sc_dt, dtype=np.float64).reshape(-1)
    assert np.array_equal(scales, sc_dt.squeeze()) and np.array_equal(freqs, row_frequencies(wav, sc, fs))
    assert torch.equal(Wx, S.ssq_cwt(x, wav, fs=fs, nv=nv)[1])
    xd = torch.as_tensor(x.astype(dtype)).to(DEV)
    W0 = _cwt.get_cwt_plan(wav, sc_dt, N, 'reflect', 1 / fs, True, 2).execute(xd, want_dWx=False)['Wx']
    Wd = _cwt.get_cwt_plan(derived_wavelets(wav)[0], sc_dt, N, 'reflect', 1 / fs, True, 2).execute(xd)['Wx']
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wav), 4.)
    gamma = 10 * R.EPS[dtype]
    assert torch.equal(Wx, W0)
    rot = S.cwt_rotation_tables(freqs, N, fs)
    assert torch.equal(Tx, S.time_reassign_cwt_gpu(W0, Wd, sc, dmax, gamma, rot=rot))
    assert not torch.equal(Tx, S.time_reassign_cwt_gpu(W0, Wd, sc, dmax, gamma, rot=False))
    assert not torch.equal(Tx, S.tssq_cwt(x, max_shift=1., **kw)[0])
    for b in range(2):
        one = S.tssq_cwt(x[b], **kw)
        assert torch.equal(one[0], Tx[b]) and torch.equal(one[1], Wx[b])
    xt = torch.as_tensor(x[0]).to(DEV).requires_grad_(True)
    Tg, Wg, _, _, t_hat = S.tssq_cwt(xt, get_t=True, **kw)
    assert all(a.grad_fn is None for a in (Tg, Wg, t_hat)) and torch.equal(Tg, Tx[0])
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    assert t_hat.shape == Wx[0].shape and t_hat.dtype == rdt
    w0, t0 = (_np(a[0]).astype(np.complex128) for a in (W0, Wd))
    th = _np(t_hat).astype(np.float64)
    low, kept = np.abs(w0) < .5 * gamma, np.abs(w0) >= 2 * gamma
    assert np.isinf(th[low]).all()
    times = np.broadcast_to(np.arange(N) / fs, w0.shape)
    r = np.broadcast_to((sc / fs)[:, None], w0.shape)
    want_t = times[kept] + (t0[kept] / w0[kept]).imag * r[kept]
    assert (np.abs(th[kept] - want_t) <= 8 * R.EPS[dtype] * (np.abs(r[kept] * t0[kept] / w0[kept]) + times.max())).all()
    outs = S.tssq_cwt(x[0], astensor=False, get_t=True, **kw)
    assert all(isinstance(a, np.ndarray) for a in outs)
    assert np.array_equal(outs[0], _np(Tx[0])) and np.array_equal(outs[1], _np(Wx[0]))
    with pytest.raises(NotImplementedError):
        S.tssq_cwt(x[0], wavelet='bump', fs=fs, nv=nv)
    with pytest.raises(NotImplementedError):
        S.tssq_cwt(x[0], wavelet=('gmw', {'order': 1}), fs=fs, nv=nv)
    with pytest.raises(ValueError, match='1D or 2D'):
        S.tssq_cwt(x[None], **kw)

    calls = []
    execute = _cwt.CwtPlan.execute

    def counted(self, *a, **k):
        calls.append(k)
        return execute(self, *a, **k)
    _cwt.CwtPlan.execute = counted
    try:
        S.tssq_cwt(x[0], **kw)
        assert calls == [dict(want_dWx=False), {}], calls
    finally:
        _cwt.CwtPlan.execute = execute


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['impulse', 'dispersive'])
def test_sharpening_against_the_restatement(S, kind, dtype, N=1024):
    """A unit impulse and a dispersive pulse (group delay linear in frequency), GMW, 16 voices, the rows between 0.06 and
    0.4 cycles per sample: the share of ``|Tx|^2`` within +-1 (+-3) columns of the true group delay of every row is
    strictly above the scalogram's, in the product and in the NumPy float64 restatement of the whole transform
    (`tssq_cwt.np_tssq`), and the product's share is within four times the difference measured on an MI355X
    (profiles/tssq_cwt.txt) of the restatement's."""
    x, wavelet, rows, tg, half = Q.e2e_case(kind, N)
    from ssqueezepy_amd import Wavelet
    wav = Wavelet((wavelet[0], dict(wavelet[1], dtype=dtype)), N=N)
    Tx, Wx, freqs, sc = S.tssq_cwt(x, wav, nv=16, fs=1.)
    assert np.allclose(freqs, Q.design(wavelet, N)[2], rtol=1e-6)
    got = Q.share(np.abs(_np(Tx).astype(np.complex128)[rows]) ** 2, tg, half)
    scal = Q.share(np.abs(_np(Wx).astype(np.complex128)[rows]) ** 2, tg, half)
    want, want_scal = Q.np_shares(kind, N)
    print('tssq_cwt %s %s N=%d: share %.12f scalogram %.6f; restatement %.12f scalogram %.6f; |difference| %.3e'
          % (kind, dtype, N, got, scal, want, want_scal, abs(got - want)))
    report_measured('tssq_cwt_%s_%s_%d' % (kind, dtype, N), share=got, scalogram=scal, restatement=want,
                    difference=abs(got - want))
    assert want > want_scal and got > scal
    assert abs(got - want) <= 4 * SHARE_MEASURED[(dtype, N)]
