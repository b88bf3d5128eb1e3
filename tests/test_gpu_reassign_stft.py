# -*- coding: utf-8 -*-
"""`reassign_stft`, `algos.reassign2d_gpu` and the entry `ssq_reassign2d` (the reassigned spectrogram: a fixed-point
scatter along both axes).

The oracle of the kernels is `reassign2d.statement`: the entry's definition in NumPy on separate real float64 arrays,
one ufunc per operation, the sum as `np.add.at` on uint64. The definition has only basic IEEE operations and the sum is
an integer sum, so `acc`, `peak` and `Rx` are compared with `==` in both dtypes. What may differ is the branch of a
point with ``|Sx|`` within 1e-6 (relative) of `gamma`, where the device's magnitude and libm's `hypot` may disagree:
every seeded case asserts that it has no such point.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import reassign2d as R
from reassign2d import _np, FS

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
SHAPE_IDS = R.SHAPE_IDS
BATCH = 9                                          # index of the batch shape
# end to end
N, N_FFT = 4096, 256


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def tile():
    """(tile rows, tile columns, halo rows, halo columns, most workgroups) of the library in use."""
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    return tuple(lib.ssq_reassign2d_tile(i) for i in range(5))


def shape_of(idx):
    shapes = R.shapes(*tile())
    assert len(shapes) == len(SHAPE_IDS)
    return shapes[idx]


_CASES = {}


def case(shape, dtype):
    """Planes and a `gamma` midway between two neighbouring samples of ``|Sx|`` near the lower quartile of the smallest
    signal, with no point near it; made once, nobody writes to them."""
    key = (shape, dtype)
    if key not in _CASES:
        Sx, dSx, Vtg = R.planes(shape, dtype)
        gamma = R.quiet_gamma(Sx)
        assert not R.near_gamma(Sx, gamma).any()
        _CASES[key] = (Sx, dSx, Vtg, gamma)
    return _CASES[key]


_REFS = {}


def reference(shape, dtype, freq=True, time=True):
    key = (shape, dtype, freq, time)
    if key not in _REFS:
        B, rows, n, dmax, kmax, _ = shape
        Sx, dSx, Vtg, gamma = case(shape, dtype)
        _REFS[key] = R.statement(Sx, dSx if freq else None, Vtg if time else None, 2 * rows, FS, FS, kmax, dmax, gamma)
    return _REFS[key]


def run(S, Sx, dSx, Vtg, shape, gamma, **kw):
    B, rows, n, dmax, kmax, _ = shape
    return S.reassign2d_gpu(Sx, dSx, Vtg, 2 * rows, 1, FS, gamma, kmax=kmax, dmax=dmax, return_acc=True, **kw)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def sync():
    import torch
    torch.cuda.synchronize() if DEV == 'cuda' else None


# ------------------------------------------------------------------------------------------ kernels against statement
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('idx', range(len(SHAPE_IDS)), ids=SHAPE_IDS)
def test_kernel_vs_statement(S, idx, dtype):
    tr, tc, hr, hc, gcap = tile()
    shape = shape_of(idx)
    B, rows, n, dmax, kmax, _ = shape
    Sx, dSx, Vtg, gamma = case(shape, dtype)
    ref = reference(shape, dtype)
    lands = ref['lands']
    if n > 1:
        assert 0 < lands.mean() < 1                         # some points are dropped, some land
    if B > 1:
        assert len(set(ref['sh'])) == B                     # a shift per signal
    # the share of the landing terms that leave the window of their tile (rows and columns)
    k = np.arange(rows)[None, :, None]
    c = np.arange(n)[None, None, :]
    out = (ref['k2'] < k // tr * tr - hr) | (ref['k2'] >= k // tr * tr + tr + hr) | \
        (ref['c2'] < c // tc * tc - hc) | (ref['c2'] >= c // tc * tc + tc + hc)
    outside = float((out & lands).sum() / max(lands.sum(), 1))
    if SHAPE_IDS[idx] == 'more_tiles_than_workgroups':
        assert B * -(-rows // tr) * -(-n // tc) > gcap
    if SHAPE_IDS[idx] == 'scattered':
        assert outside > .5
    if SHAPE_IDS[idx] in ('window_minus_1', 'past_row_halo'):
        assert 0 < outside < .5
    got = run(S, Sx, dSx, Vtg, shape, gamma)
    R.check('reassign2d_%s_%s' % (SHAPE_IDS[idx], dtype), got, ref, dtype)
    report_measured('reassign2d_kernel_%s_%s' % (SHAPE_IDS[idx], dtype), landed=float(lands.mean()),
                    outside_window=outside, filled=float((ref['acc'] != 0).mean()))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('idx', [4, 11], ids=['tile_plus_1', 'scattered'])
def test_no_window_and_repeat_give_the_same_bits(S, idx, dtype):
    """Two launches, and the launch that sends every term through a global atomic, are `torch.equal`."""
    import torch
    shape = shape_of(idx)
    Sx, dSx, Vtg, gamma = case(shape, dtype)
    a = run(S, Sx, dSx, Vtg, shape, gamma)
    for other in (run(S, Sx, dSx, Vtg, shape, gamma), run(S, Sx, dSx, Vtg, shape, gamma, window=False)):
        assert all(torch.equal(x, y) for x, y in zip(a, other))
    R.check('reassign2d_no_window_%d_%s' % (idx, dtype), run(S, Sx, dSx, Vtg, shape, gamma, window=False),
            reference(shape, dtype), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_permuted_columns_give_the_same_bits(S, dtype):
    """The planes with their columns reversed and the group delays negated are the same scatter walked the other way
    round: the result is the reversed result, bit for bit."""
    import torch
    shape = shape_of(4)
    Sx, dSx, Vtg, gamma = case(shape, dtype)
    a = run(S, Sx, dSx, Vtg, shape, gamma)
    b = run(S, Sx[..., ::-1], dSx[..., ::-1], -Vtg[..., ::-1], shape, gamma)
    assert torch.equal(a[0].flip(-1), b[0]) and torch.equal(a[1].flip(-1), b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls(S, dtype):
    import torch
    shape = shape_of(BATCH)
    Sx, dSx, Vtg, gamma = case(shape, dtype)
    Sd, Dd, Vd = dev(Sx), dev(dSx), dev(Vtg)
    Rx, acc, peak = run(S, Sd, Dd, Vd, shape, gamma)
    for b in range(shape[0]):
        one = run(S, Sd[b], Dd[b], Vd[b], shape, gamma)
        assert one[0].shape == Rx.shape[1:]
        assert torch.equal(one[0], Rx[b]) and torch.equal(one[1], acc[b]) and torch.equal(one[2], peak[b:b + 1]), b


# ------------------------------------------------------------------------------------------ crafted planes
def crafted_run(S, amp, m, d, dtype, n_fft, kmax, dmax, gamma=0.):
    Sx, dSx, Vtg = R.crafted(amp, m, d, dtype, n_fft)
    ref = R.statement(Sx, dSx, Vtg, n_fft, FS, FS, kmax, dmax, gamma)
    got = S.reassign2d_gpu(Sx, dSx, Vtg, n_fft, 1, FS, gamma, kmax=kmax, dmax=dmax, return_acc=True)
    R.check('reassign2d_crafted', got, ref, dtype)
    return _np(got[0]).astype(np.float64), _np(got[1]).view(np.uint64), ref


@pytest.mark.parametrize('dtype', DTYPES)
def test_identity_and_uniform_shift(S, dtype):
    rng = np.random.default_rng(5)
    rows, n, n_fft = 7, 300, 16
    amp = 1. + rng.random((1, rows, n))
    e = (amp.astype(dtype).astype(np.float64)) ** 2
    Rx, _, ref = crafted_run(S, amp, 0, 0, dtype, n_fft, 3, 40)
    # a term loses less than 2^-sh to the truncation, and the cell is rounded once to the data type
    tol = 2. ** -ref['sh'][0] + R.EPS[dtype] * e.max()
    assert np.abs(Rx - e).max() <= tol
    Rx, acc, ref = crafted_run(S, amp, 2, -37, dtype, n_fft, 3, 40)
    want = np.zeros_like(e)
    want[:, 2:, :n - 37] = e[:, :rows - 2, 37:]                     # rows past the last one and columns past the left end drop
    assert np.array_equal(Rx != 0, want != 0)
    assert np.abs(Rx - want).max() <= tol


@pytest.mark.parametrize('dtype', DTYPES)
def test_reflection_and_drops(S, dtype):
    """Row displacements that cross row 0 come back reflected; a point is dropped past the last row, past `kmax`, past
    `dmax` and past either column end. One point per row, every other point below `gamma`."""
    rows, n, n_fft, kmax, dmax = 8, 50, 16, 5, 10
    amp = np.full((1, rows, n), 1e-3)
    m, d = np.zeros((1, rows, n)), np.zeros((1, rows, n))
    #        row col   m    d      lands at
    pts = [(1, 20, -3, 0),       # (2, 20): reflected at row 0
           (2, 20, -2, 1),       # (0, 21)
           (6, 20, 3, 0),        # row 9: past the last row
           (0, 20, 6, 0),        # past kmax
           (3, 20, 0, 11),       # past dmax
           (4, 3, 0, -5),        # past the left end
           (5, 47, 0, 4),        # past the right end
           (7, 5, -5, 10)]       # (2, 15)
    for k, c, mm, dd in pts:
        amp[0, k, c], m[0, k, c], d[0, k, c] = 2. + k, mm, dd
    Rx, acc, ref = crafted_run(S, amp, m, d, dtype, n_fft, kmax, dmax, gamma=.5)
    want = np.zeros((1, rows, n))
    want[0, 2, 20], want[0, 0, 21], want[0, 2, 15] = 9., 16., 81.
    assert np.array_equal(Rx, want)
    assert ref['peak'][0] == np.float64(81.).view(np.uint64)


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_point_into_one_cell_pins_the_headroom(S, dtype):
    """Every point of the plane goes to one cell, every energy equal to the peak, ``n = 2 dmax + 1``: the cell holds
    ``C q`` exactly, below 2^62 and above 2^60 -- one bit less of headroom would overflow, one more would waste it."""
    rows, dmax = 9, 35
    n, n_fft = 2 * dmax + 1, 32
    k, c = np.arange(rows)[None, :, None], np.arange(n)[None, None, :]
    for amp in (1., 1.5, 3e-9):
        Rx, acc, ref = crafted_run(S, amp, 4 - k, dmax - c, dtype, n_fft, rows, dmax)
        C = rows * n
        q = int(ref['q'].max())
        assert int(acc[0, 4, dmax]) == C * q and np.count_nonzero(acc) == 1
        assert 2 ** 60 <= C * q < 2 ** 62
        assert R.cell_terms(rows, n, dmax) == C


@pytest.mark.parametrize('dtype', DTYPES)
def test_points_below_gamma_and_non_finite_points(S, dtype):
    """Points below `gamma`, a NaN and an Inf point contribute nothing and do not set the peak; an all-zero signal in a
    batch gives zeros and leaves its neighbours alone."""
    rows, n, n_fft = 4, 70, 8
    rng = np.random.default_rng(9)
    amp = 1. + rng.random((3, rows, n))
    amp[1] = 0.
    amp[0, 1, 5], amp[0, 2, 6], amp[0, 3, 7] = np.nan, np.inf, 100.       # (100 is kept: the peak of signal 0)
    amp[2, 0, :10] = 1e-3
    m = rng.integers(-1, 2, (3, rows, n))
    d = rng.integers(-3, 4, (3, rows, n))
    with np.errstate(all='ignore'):
        Rx, acc, ref = crafted_run(S, amp, m, d, dtype, n_fft, 1, 3, gamma=.5)
    assert ref['peak'][0] == np.float64(1e4).view(np.uint64) and ref['peak'][1] == 0
    assert not Rx[1].any() and Rx[0].any() and Rx[2].any() and np.isfinite(Rx).all()
    # signal 2 without its points below gamma, alone: the same bits
    amp2 = amp[2:].copy()
    amp2[0, 0, :10] = 0.
    alone, _, _ = crafted_run(S, amp2, m[2:], d[2:], dtype, n_fft, 1, 3, gamma=.5)
    assert np.array_equal(alone[0], Rx[2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_order_independence_where_a_float_sum_fails(S, dtype):
    """One cell receives a term of 1 and then 1024 terms of 2^-30: a running float32 sum stays at 1, the fixed-point
    sum is ``1 + 2^-20`` exactly, in either order of the sources."""
    n, n_fft = 1025, 4
    c = np.arange(n)[None, None, :]
    amp = np.where(c == 0, 1., 2. ** -15)
    s = np.float32(1.)
    for _ in range(1024):
        s = np.float32(s + np.float32(2. ** -30))
    assert s == 1.
    for target, a in ((0, amp), (n - 1, amp[..., ::-1])):
        Rx, acc, ref = crafted_run(S, a, 0, target - c, dtype, n_fft, 0, n - 1)
        assert Rx[0, 0, target] == 1. + 2. ** -20 and np.count_nonzero(Rx) == 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_conservation_and_links(S, dtype):
    """`acc` sums to the `q` of the points that land, as integers. ``'time'``: the statement with ``m = 0``, and the
    landing cells are `time_reassign_gpu`'s on the same planes (on ``|Sx|^2``: the next test); ``'freq'``: nothing
    crosses a column."""
    shape = shape_of(BATCH)
    B, rows, n, dmax, kmax, _ = shape
    Sx, dSx, Vtg, gamma = case(shape, dtype)
    for freq, time in ((True, True), (False, True), (True, False)):
        ref = reference(shape, dtype, freq, time)
        got = run(S, Sx, dSx if freq else None, Vtg if time else None, shape, gamma)
        R.check('reassign2d_links_%d%d_%s' % (freq, time, dtype), got, ref, dtype)
        acc = _np(got[1]).view(np.uint64)
        for b in range(B):
            assert sum(map(int, acc[b].reshape(-1))) == sum(map(int, ref['q'][b][ref['lands'][b]]))
        if not time:
            want = np.where(ref['lands'], ref['q'], np.uint64(0)).astype(object).sum(axis=1)
            assert np.array_equal(acc.astype(object).sum(axis=1), want)
            assert np.array_equal(_np(run(S, Sx, dSx, Vtg, shape[:3] + (0,) + shape[4:], gamma)[1]),
                                  _np(got[1]))                        # dmax = 0 with Vtg given: the same
        if not freq:
            assert (ref['k2'] == np.arange(rows)[None, :, None]).all()
            Tx = _np(S.time_reassign_gpu(Sx, Vtg, 2 * rows, 1, FS, gamma, rot=False, dmax=dmax))
            assert np.array_equal(Tx != 0, acc != 0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_time_mode_has_the_geometry_of_time_reassign_on_the_energy(S, dtype):
    """``reassign='time'`` against `time_reassign_gpu` run on the plane ``|Sx|^2`` itself (no rotation): crafted planes
    with integer group delays, so both take the same displacements; the inputs of the sibling are real and non-negative,
    so nothing cancels and the landing cells are the same set; and the sibling's float64 sums are the fixed-point sums to
    within the terms' truncation, ``terms 2^-sh``, plus the roundings of `dtype`: of the energy plane, of the cell, and of
    a running sum of at most ``2 dmax + 1`` terms."""
    rng = np.random.default_rng(21)
    rows, n, n_fft, dmax = 6, 300, 16, 15
    amp = 1. + rng.random((1, rows, n))
    amp[rng.random((1, rows, n)) < .2] = 1e-3                       # below gamma in both forms
    d = rng.integers(-20, 21, (1, rows, n))                         # some beyond dmax, some past a column end
    Sx, _, Vtg = R.crafted(amp, 0, d, dtype, n_fft)
    ref = R.statement(Sx, None, Vtg, n_fft, FS, FS, 0, dmax, .5)
    got = S.reassign2d_gpu(Sx, None, Vtg, n_fft, 1, FS, .5, dmax=dmax, return_acc=True)
    R.check('reassign2d_time_link_%s' % dtype, got, ref, dtype)
    Rx, acc = _np(got[0]).astype(np.float64), _np(got[1])
    E, _, VtgE = R.crafted(Sx.real.astype(np.float64) ** 2, 0, d, dtype, n_fft)
    Tx = _np(S.time_reassign_gpu(E, VtgE, n_fft, 1, FS, .25, rot=False, dmax=dmax)).astype(np.complex128)
    assert 0 < ref['lands'].mean() < 1 and (np.bincount(ref['c2'][ref['lands']]) > 0).any()
    assert not Tx.imag.any() and (Tx.real >= 0).all()
    assert np.array_equal(Tx.real != 0, acc != 0)
    terms = 2 * dmax + 1
    tol = terms * 2. ** -ref['sh'][0] + (terms + 2) * R.EPS[dtype] * Rx.max()
    assert np.abs(Tx.real - Rx).max() <= tol


# ------------------------------------------------------------------------------------------ layouts and refusals
@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """`out=`, strided and lazily conjugated views and NumPy planes give the bits of the plain planes; so do pointers
    that are only 8-byte aligned, through the entry itself (the element-load instance in both dtypes)."""
    import torch
    from ssqueezepy_amd import _lib, algos
    shape = shape_of(BATCH)
    B, rows, n, dmax, kmax, _ = shape
    Sx, dSx, Vtg, gamma = case(shape, dtype)
    Sd, Dd, Vd = dev(Sx), dev(dSx), dev(Vtg)
    want, want_acc, _ = run(S, Sd, Dd, Vd, shape, gamma)
    big = torch.zeros((B, rows, n + 3), dtype=Sd.dtype, device=DEV)
    big[..., 1:-2] = Sd
    conj = dev(np.conj(Vtg)).conj()
    assert conj.is_conj() and not big[..., 1:-2].is_contiguous()
    assert torch.equal(run(S, big[..., 1:-2], Dd, conj, shape, gamma)[0], want)
    assert torch.equal(run(S, Sx, dSx, Vtg, shape, gamma)[0], want)          # NumPy planes
    out = torch.full_like(want, -7.)
    assert run(S, Sd, Dd, Vd, shape, gamma, out=out)[0] is out and torch.equal(out, want)
    with pytest.raises(ValueError, match='`out`'):
        run(S, Sd, Dd, Vd, shape, gamma, out=out[..., ::2])
    with pytest.raises(ValueError, match='`out`'):
        run(S, Sd, Dd, Vd, shape, gamma, out=torch.zeros_like(Sd))
    with pytest.raises(ValueError, match='share one shape'):
        run(S, Sd, Dd[..., :-1], Vd, shape, gamma)
    with pytest.raises(TypeError):
        run(S, Sd.real, Dd, Vd, shape, gamma)

    # every plane 8 bytes past a 16-byte boundary: real buffers, the planes from their second element on
    lib = _lib.load()
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    step = 8 // (4 if dtype == 'float32' else 8)                           # reals in 8 bytes
    bufs = []
    for src in (Sd, Dd, Vd):
        buf = torch.zeros(2 * src.numel() + step, dtype=rdt, device=DEV)
        buf[step:] = torch.view_as_real(src).reshape(-1)
        assert buf.data_ptr() % 16 == 0
        bufs.append(buf)
    Rx = torch.full((B, rows, n), -7., dtype=rdt, device=DEV)
    acc = torch.zeros((B, rows, n), dtype=torch.int64, device=DEV)
    peak = torch.zeros((B,), dtype=torch.int64, device=DEV)
    rc = lib.ssq_reassign2d(_lib.F32 if dtype == 'float32' else _lib.F64, bufs[0].data_ptr() + 8, bufs[1].data_ptr() + 8,
                            bufs[2].data_ptr() + 8, Rx.data_ptr(), acc.data_ptr(), peak.data_ptr(), B, rows, n, 2 * rows,
                            1, FS, FS, kmax, dmax, float(gamma), _lib.REASSIGN2D_FREQ, algos.stream())
    assert rc == 0, lib.ssq_last_error()
    sync()
    assert torch.equal(Rx, want) and torch.equal(acc, want_acc)


def test_abi_refusals_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert lib.ssq_version() >= 115 and _lib.ABI_VERSION >= 115 and 'ssq_reassign2d' in _lib.EXPORTS
    tr, tc, hr, hc, gcap = tile()
    assert tr >= 1 and tc >= 64 and hr >= 0 and hc >= 0 and gcap >= 1 and lib.ssq_reassign2d_tile(5) == 0
    max_dmax = lib.ssq_time_reassign_max_dmax()
    B, rows, n, n_fft = 1, 5, 11, 8
    Sx, dSx, Vtg = R.planes((B, rows, n, 4, 1, 2), 'float64')
    Sd, Dd, Vd = dev(Sx), dev(dSx), dev(Vtg)
    Rx = torch.full((B, rows, n), -7., dtype=torch.float64, device=DEV)
    acc = torch.full((B, rows, n), -7, dtype=torch.int64, device=DEV)
    peak = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    good = dict(Sx=Sd.data_ptr(), dSx=Dd.data_ptr(), Vtg=Vd.data_ptr(), Rx=Rx.data_ptr(), acc=acc.data_ptr(),
                peak=peak.data_ptr(), batch=B, rows=rows, n=n, n_fft=n_fft, hop=1, fs=FS, cps=FS, kmax=1, dmax=4, gamma=.5,
                flags=_lib.REASSIGN2D_FREQ)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ssq_reassign2d(_lib.F64, a['Sx'], a['dSx'], a['Vtg'], a['Rx'], a['acc'], a['peak'], a['batch'],
                                  a['rows'], a['n'], a['n_fft'], a['hop'], a['fs'], a['cps'], a['kmax'], a['dmax'],
                                  a['gamma'], a['flags'], None)
    nan, inf = float('nan'), float('inf')
    refused = [dict(Sx=None), dict(dSx=None), dict(Vtg=None), dict(Rx=None), dict(acc=None), dict(peak=None),
               dict(batch=0), dict(rows=0), dict(n=0), dict(batch=1 << 20, rows=64, n=64, n_fft=64), dict(n_fft=0),
               dict(hop=0), dict(rows=9), dict(dmax=-1), dict(dmax=max_dmax + 1), dict(kmax=-1), dict(fs=0.), dict(fs=-1.),
               dict(fs=inf), dict(fs=nan), dict(cps=0.), dict(cps=-1.), dict(cps=inf), dict(cps=nan), dict(gamma=-1.),
               dict(gamma=nan), dict(flags=4)]
    # (rows * min(2 dmax + 1, n) >= 2^40 cannot be reached: it is at most rows * n, which the point count keeps below 2^32)
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_reassign2d'), (kw, lib.ssq_last_error())
        assert bool((Rx == -7.).all()) and bool((acc == -7).all()) and bool((peak == -7).all()), kw
    assert call() == 0
    assert call(dSx=None, flags=0) == 0 and call(Vtg=None, dmax=0) == 0 and call(kmax=1 << 40, dmax=max_dmax) == 0
    sync()
    assert not bool((Rx == -7.).any()) and not bool((acc == -7).any())


# ------------------------------------------------------------------------------------------ end to end
def signal(N):
    t = np.arange(N)
    rng = np.random.default_rng(11)
    return np.cos(2 * np.pi * (.11 * t + 1e-4 * t * t)) + (np.abs(t - N // 2) < 3) * 4. + .1 * rng.standard_normal(N)


def tau_plane(S, x, g, hop, fs, dtype):
    """The STFT with window ``tau g`` from a plan of its own."""
    import torch
    from ssqueezepy_amd import _stft
    n_fft = len(g)
    tau = (np.arange(n_fft) - n_fft // 2) / fs
    xd = torch.as_tensor(np.asarray(x).astype(dtype)).to(DEV)
    B = 1 if x.ndim == 1 else x.shape[0]
    return _stft.get_stft_plan(x.shape[-1], n_fft, hop, tau * g.astype(dtype).astype('float64'), None, fs, 'reflect',
                               True, dtype, B).execute(xd)['Sx']


@pytest.mark.parametrize('hop', [1, 4])
@pytest.mark.parametrize('dtype', DTYPES)
def test_reassign_stft_is_its_parts(S, dtype, hop, N=1024):
    """`Sx` is `stft`'s, `Rx` is `reassign2d_gpu` on separately executed plans; a batch is its single calls; `get_maps`;
    ``astensor=False``; the three modes."""
    import torch
    n_fft = 128
    g, fs = R.gauss_window(n_fft, n_fft / 12.), 50.
    x = np.stack([signal(N), 1e2 * signal(N)[::-1].copy()])
    kw = dict(window=g, n_fft=n_fft, hop_len=hop, fs=fs, dtype=dtype)
    Rx, Sx, Sfs, times = S.reassign_stft(x, **kw)
    n = (N - 1) // hop + 1
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    assert Rx.shape == Sx.shape == (2, n_fft // 2 + 1, n) and Rx.dtype == rdt and not Rx.requires_grad
    assert np.array_equal(Sfs, np.linspace(0, .5 * fs, n_fft // 2 + 1, dtype=dtype))
    assert times.dtype == np.dtype(dtype) and np.array_equal(times, (np.arange(n) * hop / fs).astype(dtype))
    S0, dS0 = S.stft(x, derivative=True, **kw)
    assert torch.equal(Sx, S0)
    Vtg = tau_plane(S, x, g, hop, fs, dtype)
    gamma = 10 * R.EPS[dtype]
    assert torch.equal(Rx, S.reassign2d_gpu(Sx, dS0, Vtg, n_fft, hop, fs, gamma))
    Rf = S.reassign_stft(x, reassign='freq', **kw)[0]
    Rt, St = S.reassign_stft(x, reassign='time', **kw)[:2]           # (one plan output: `stft`'s without the derivative)
    assert torch.equal(St, S.stft(x, **kw))
    assert torch.equal(Rf, S.reassign2d_gpu(Sx, dS0, None, n_fft, hop, fs, gamma))
    assert torch.equal(Rt, S.reassign2d_gpu(St, None, Vtg, n_fft, hop, fs, gamma))
    assert not torch.equal(Rf, Rx) and not torch.equal(Rt, Rx)
    for b in range(2):
        one = S.reassign_stft(x[b], **kw)
        assert torch.equal(one[0], Rx[b]) and torch.equal(one[1], Sx[b])
    xt = torch.as_tensor(x[0]).to(DEV).requires_grad_(True)
    Rg, Sg, _, _, f_hat, t_hat = S.reassign_stft(xt, get_maps=True, **kw)
    assert all(a.grad_fn is None for a in (Rg, Sg, f_hat, t_hat)) and torch.equal(Rg, Rx[0])
    assert f_hat.shape == t_hat.shape == Sx[0].shape
    sx = _np(Sx[0]).astype(np.complex128)
    ds, vt = _np(dS0[0]).astype(np.complex128), _np(Vtg[0]).astype(np.complex128)
    fh, th = _np(f_hat).astype(np.float64), _np(t_hat).astype(np.float64)
    low, kept = np.abs(sx) < .5 * gamma, np.abs(sx) >= 2 * gamma
    assert np.isinf(fh[low]).all() and np.isinf(th[low]).all()
    want_f = np.broadcast_to(Sfs.astype(np.float64)[:, None], sx.shape)[kept] - (ds[kept] / sx[kept]).imag / (2 * np.pi)
    want_t = np.broadcast_to(times.astype(np.float64), sx.shape)[kept] + (vt[kept] / sx[kept]).real
    assert (np.abs(fh[kept] - want_f) <= 8 * R.EPS[dtype] * (np.abs(ds[kept] / sx[kept]) + .5 * fs)).all()
    assert (np.abs(th[kept] - want_t) <= 8 * R.EPS[dtype] * (np.abs(vt[kept] / sx[kept]) + times.max())).all()
    one = S.reassign_stft(x[0], reassign='freq', get_maps=True, **kw)
    assert one[5] is None and one[4] is not None
    outs = S.reassign_stft(x[0], astensor=False, get_maps=True, **kw)
    assert all(isinstance(a, np.ndarray) for a in outs)
    assert np.array_equal(outs[0], _np(Rx[0])) and np.array_equal(outs[1], _np(Sx[0]))
    with pytest.raises(ValueError, match='`reassign`'):
        S.reassign_stft(x[0], reassign='neither', **kw)


@pytest.mark.parametrize('hop', [1, 8])
@pytest.mark.parametrize('dtype', DTYPES)
def test_fm_tone_shares_are_ordered(S, dtype, hop):
    """A frequency-modulated tone, ``0.25 + 0.08 cos(2 pi t / 600)`` cycles per sample, Gaussian window of sigma 24: the
    share of the energy within +-1 row of the true frequency is strictly ordered, spectrogram < 'freq' < 'time' <
    'both', and 'both' is above 0.9. With `reassign2d.ridge_share` -- the true row is ``rint(f n_fft)`` at the column's
    time -- the product gives 0.470 / 0.569 / 0.951 / 0.998 at hop 1 and 0.470 / 0.568 / 0.943 / 0.998 at hop 8, in both
    dtypes; the four shares are printed."""
    x, f = R.fm_tone(N)
    kw = dict(window=R.gauss_window(N_FFT, 24.), n_fft=N_FFT, hop_len=hop, fs=1., dtype=dtype)
    shares = {}
    for mode in ('freq', 'time', 'both'):
        Rx, Sx, _, _ = S.reassign_stft(x, reassign=mode, **kw)
        shares[mode] = R.ridge_share(Rx, f, N_FFT, hop)
    shares['spectrogram'] = R.ridge_share(np.abs(_np(Sx)).astype(np.float64) ** 2, f, N_FFT, hop)
    print('fm tone %s hop %d: spectrogram %.4f freq %.4f time %.4f both %.4f' % (
        dtype, hop, shares['spectrogram'], shares['freq'], shares['time'], shares['both']))
    report_measured('reassign_fm_tone_%s_hop%d' % (dtype, hop), **shares)
    assert shares['spectrogram'] < shares['freq'] < shares['time'] < shares['both']
    assert shares['both'] > .9


@pytest.mark.parametrize('dtype', DTYPES)
def test_impulse_column_share(S, dtype, N=1024):
    """A unit impulse: with 'both' its column holds a larger share of the energy than with 'freq'."""
    x = np.zeros(N)
    x[400] = 1.
    kw = dict(window=R.gauss_window(128, 128 / 12.), n_fft=128, hop_len=1, fs=1., dtype=dtype)
    share = {}
    for mode in ('freq', 'both'):
        E = _np(S.reassign_stft(x, reassign=mode, **kw)[0]).astype(np.float64)
        share[mode] = float(E[:, 400].sum() / E.sum())
    report_measured('reassign_impulse_%s' % dtype, **share)
    assert share['both'] > share['freq']
