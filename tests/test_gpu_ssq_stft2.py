# -*- coding: utf-8 -*-
"""`ssq_stft2`: the second-order synchrosqueezed STFT (`ssq_stft2_phase` + the ordered
reassignment), DESIGN.md section 4.5.3.

The oracle of the map is `statement` below: the definition, written in NumPy, evaluated in
float64 (the reference) and again in `np.clongdouble`. `E`, the largest difference between the two
evaluations over the finite points, is the reference's own rounding error; the device -- float64
arithmetic per point, products possibly associated otherwise -- must agree with the float64
evaluation to `8 E + spacing(w_ref)` in the output dtype, and on every `inf`. (Where a float32 point falls
back to the first order the kernel hands out `phase_stft`'s value, float32 numerator included; the tests of
`chirp_tol=inf` use that form of the statement, `first_order_float32`.) Points within 1e-6
(relative) of one of the two thresholds may fall on either side and are left out; there may be at
most 1e-4 of them.

What the map is *for* is checked on a linear chirp, against a NumPy float64 restatement of the
whole transform (STFTs included): `ssq_stft2` puts the interior energy into the bin of the true
instantaneous frequency, `ssq_stft` does not.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import second_order
from second_order import _np, default_gamma

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
TWO_PI = 6.283185307179586                 # the float64 constant of the definition
MAP_SHAPES = [(777, 128, 1), (1000, 96, 4), (640, 256, 16)]      # (N, n_fft, hop)
FS = 200.


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def gauss(n_fft, div):
    return np.exp(-.5 * ((np.arange(n_fft) - n_fft // 2) / (n_fft / div))**2)


def two_chirps_fs(N, seed=0):
    t = np.arange(N) / FS
    noise = np.random.default_rng(seed).standard_normal(N)
    return (np.cos(2 * np.pi * (10 * t + 6 * t**2)) + .7 * np.cos(2 * np.pi * (80 * t - 4.5 * t**2))
            + .05 * noise)


def first_order_float32(Vg, Vdg, Sfs):
    """`|Re(w1c)|` as `phase_stft` evaluates it for complex64 data, the reference's CPU arithmetic:
    ``Im(dSx conj(Sx))`` and ``|Sx|^2`` in float32, float64 from the 2 pi on."""
    a, b, c, d = Vdg.real, Vdg.imag, Vg.real, Vg.imag
    assert a.dtype == np.float32
    with np.errstate(all='ignore'):
        num, m2 = b * c - a * d, c * c + d * d
        r = num.astype(np.float64) / (m2.astype(np.float64) * TWO_PI)
    return np.abs(np.asarray(Sfs, dtype=np.float64)[:, None] - r)


def statement(Vg, Vdg, Vddg, Vtg, Vtdg, Sfs, gamma, chirp_tol, ctype=np.complex128, fallback32=False):
    """The definition, operation by operation, in `ctype`. Returns `w` (not yet rounded to an output
    dtype) and the two threshold quantities ``|den| / |Vg|^2`` and ``|Vg|``. `fallback32`: the points
    that fall back to the first order carry `phase_stft`'s value for complex64 data
    (`first_order_float32`), which is what the kernel hands out there."""
    w1_32 = first_order_float32(Vg, Vdg, Sfs) if fallback32 else None
    rtype = np.float64 if ctype == np.complex128 else np.longdouble
    Vg, Vdg, Vddg, Vtg, Vtdg = [np.asarray(V).astype(ctype) for V in (Vg, Vdg, Vddg, Vtg, Vtdg)]
    Sfs = np.asarray(Sfs).astype(rtype)[:, None]
    two_pi = rtype(TWO_PI)
    with np.errstate(all='ignore'):
        r = Vdg / Vg
        w1c = Sfs + ctype(1j) * r / two_pi
        den = Vtg * Vdg - Vtdg * Vg
        q = (Vddg * Vg - Vdg * Vdg) / den / (two_pi * ctype(1j))
        w2 = (w1c - q * Vtg / Vg).real
        aVg = np.abs(Vg)
        ratio = np.abs(den) / aVg**2
        second = np.abs(den) > rtype(chirp_tol) * aVg**2
        w = np.where(second, np.abs(w2), np.abs(w1c.real) if w1_32 is None else w1_32.astype(rtype))
        w = np.where(aVg < rtype(gamma), rtype(np.inf), w)
    return w, ratio, aVg


def check_map(name, w_dev, planes, Sfs, gamma, chirp_tol, rdtype, fallback32=False):
    """`second_order.check_map` on this module's `statement`; with `fallback32` the reference carries
    `phase_stft`'s float32 first-order value at the points that fall back."""
    ref = statement(*planes, Sfs, gamma, chirp_tol, fallback32=True)[0] if fallback32 else None
    return second_order.check_map(name, w_dev, statement(*planes, Sfs, gamma, chirp_tol),
                                  statement(*planes, Sfs, gamma, chirp_tol, np.clongdouble), gamma, chirp_tol, rdtype,
                                  ref)


_PLANES = {}


def five_planes(S, N, n_fft, hop, dtype, batch=None):
    """The five transforms of the test signal (host arrays), from the package's own STFT plans with the
    window pairs `ssq_stft2` uses; computed once per configuration and shared; nobody writes to them."""
    key = (N, n_fft, hop, dtype, batch)
    if key not in _PLANES:
        from ssqueezepy_amd import _stft, _ssq_stft2
        x = (two_chirps_fs(N) if batch is None else
             np.stack([two_chirps_fs(N, seed=s) * (1 + s) for s in range(batch)]))
        g = gauss(n_fft, 10)
        Sx, dSx = S.stft(x, window=g, n_fft=n_fft, hop_len=hop, fs=FS, derivative=True, dtype=dtype)
        win, dwin = _stft.get_window(g, n_fft, n_fft, derivative=True, dtype=dtype)
        planes = [Sx, dSx]
        import torch
        xd = torch.as_tensor(x.astype(dtype), device=DEV)
        for k, (wa, wb) in enumerate(_ssq_stft2._second_order_windows(win, dwin, n_fft, FS)):
            plan = _stft.get_stft_plan(N, n_fft, hop, wa, wb, FS, 'reflect', True, dtype,
                                       1 if batch is None else batch)
            out = plan.execute(xd, want_dSx=True)
            planes += [out['Sx'], out['dSx']] if k == 0 else [out['dSx']]
        Vg, Vdg, Vtg, Vtdg, Vddg = [_np(p) for p in planes]
        _PLANES[key] = (x, (Vg, Vdg, Vddg, Vtg, Vtdg), np.linspace(0, .5 * FS, n_fft // 2 + 1, dtype=dtype))
    return _PLANES[key]


# ---------------------------------------------------------------- 1. the map
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', MAP_SHAPES + [(1000, 96, 4, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_map_vs_numpy_statement(S, shape, dtype):
    N, n_fft, hop = shape[:3]
    batch = shape[3] if len(shape) == 4 else None
    _, planes, Sfs = five_planes(S, N, n_fft, hop, dtype, batch)
    gamma = default_gamma(dtype)
    w = S.phase_stft2_gpu(*planes, Sfs, gamma, 1e-3)
    assert tuple(w.shape) == planes[0].shape and str(w.dtype).endswith(dtype)
    if batch is None:
        check_map('stft2_map-%s-%s' % ('x'.join(map(str, shape)), dtype), _np(w), planes, Sfs, gamma, 1e-3,
                  np.dtype(dtype))
    else:
        for b in range(batch):
            check_map('stft2_map-%s-%s[%d]' % ('x'.join(map(str, shape)), dtype, b), _np(w)[b],
                      [p[b] for p in planes], Sfs, gamma, 1e-3, np.dtype(dtype))


# ------------------------------------------------- 2. Tx = ordered reassignment
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('flipud', [False, True])
def test_tx_is_ordered_reassignment_of_w(S, dtype, flipud, N=777, n_fft=128, hop=1, B=3):
    import torch
    g = gauss(n_fft, 10)
    xb = np.stack([two_chirps_fs(N, seed=s) * (1 + s) for s in range(B)])
    kw = dict(window=g, n_fft=n_fft, hop_len=hop, fs=FS, dtype=dtype)
    singles = []
    for x in (xb[1], xb):
        Tx, Sx, ssq_freqs, Sfs, w = S.ssq_stft2(x, flipud=flipud, get_w=True, **kw)
        assert Tx.shape == Sx.shape == w.shape == x.shape[:-1] + (n_fft // 2 + 1, (N - 1) // hop + 1)
        assert Tx.grad_fn is None and Sx.grad_fn is None
        grid = ssq_freqs[::-1] if flipud else ssq_freqs       # returned flipped; the kernels take it ascending
        const = grid[1] - grid[0]
        assert torch.equal(Tx, S.indexed_sum_onfly(Sx, w, grid, const, False, flipud))
        again = S.ssq_stft2(x, flipud=flipud, get_w=True, **kw)
        assert torch.equal(Tx, again[0]) and torch.equal(w, again[4]) and torch.equal(Sx, again[1])
        assert torch.equal(Sx, S.ssq_stft(x, flipud=flipud, **kw)[1])
        singles.append((Tx, Sx, w))
    (T1, S1, w1), (Tb, Sb, wb) = singles
    assert torch.equal(Tb[1], T1) and torch.equal(Sb[1], S1) and torch.equal(wb[1], w1)
    assert float(torch.abs(T1).max()) > 0


# ------------------------------------------------------- 3. what it is for
def np_stft(x, h, n_fft):
    """`V^h` of the definition in float64: reflect padding, hop 1, frame times `h`, ifftshift, rfft."""
    xp = np.pad(x, (n_fft // 2, n_fft - n_fft // 2 - 1), mode='reflect')
    frames = np.lib.stride_tricks.sliding_window_view(xp, n_fft)             # (N, n_fft)
    return np.fft.rfft(np.fft.ifftshift(frames * h, axes=-1), axis=-1).T     # (rows, N)


def np_reassign(Sx, w, ssq_freqs):
    """`indexed_sum_onfly` on the linear grid, in NumPy (sums in float64, ascending rows)."""
    const = ssq_freqs[1] - ssq_freqs[0]
    Tx = np.zeros(Sx.shape, dtype=np.complex128)
    ok = np.isfinite(w)
    k = np.clip(np.rint((np.where(ok, w, 0) - ssq_freqs[0]) / const), 0, len(ssq_freqs) - 1).astype(int)
    for i in range(Sx.shape[0]):
        cols = np.nonzero(ok[i])[0]
        np.add.at(Tx, (k[i, cols], cols), Sx[i, cols] * const)
    return Tx


def ridge_share(Tx, bins, cols):
    E = np.abs(Tx[:, cols])**2
    return float(E[bins[cols], np.arange(len(cols))].sum() / E.sum())


_CHIRP = {}


def chirp_reference(N=2048, n_fft=256, rate=2e-4, f0=.05):
    """The chirp of the issue and the NumPy float64 restatement of both transforms on it: the shares of
    the interior energy in the bin of the true instantaneous frequency (computed once)."""
    if not _CHIRP:
        from ssqueezepy_amd._stft import _spectral_derivative as D
        n = np.arange(N)
        x = np.cos(2 * np.pi * (f0 * n + .5 * rate * n**2))
        g = gauss(n_fft, 12)
        tau = (np.arange(n_fft) - n_fft // 2) / 1.
        dg = D(g)
        V = [np_stft(x, h, n_fft) for h in (g, dg, D(dg), tau * g, tau * dg)]
        Sfs = np.linspace(0, .5, n_fft // 2 + 1)
        gamma = default_gamma('float64')
        w2, _, _ = statement(*V, Sfs, gamma, 1e-3)
        w1, _, _ = statement(*V, Sfs, gamma, np.inf)
        bins = np.rint((f0 + rate * n) * n_fft).astype(int)
        cols = np.arange(n_fft, N - n_fft)
        _CHIRP.update(x=x, g=g, bins=bins, cols=cols, n_fft=n_fft,
                      share2=ridge_share(np_reassign(V[0], w2, Sfs), bins, cols),
                      share1=ridge_share(np_reassign(V[0], w1, Sfs), bins, cols))
    return _CHIRP


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_sharpens_a_linear_chirp(S, dtype):
    ref = chirp_reference()
    # the oracle itself: exact for a linear chirp under a Gaussian window up to the window's truncation
    assert ref['share2'] > 0.99, ref['share2']
    kw = dict(window=ref['g'], n_fft=ref['n_fft'], hop_len=1, fs=1., dtype=dtype)
    share2 = ridge_share(_np(S.ssq_stft2(ref['x'], **kw)[0]), ref['bins'], ref['cols'])
    share1 = ridge_share(_np(S.ssq_stft(ref['x'], **kw)[0]), ref['bins'], ref['cols'])
    report_measured('stft2_chirp_share-' + dtype, ssq_stft2=share2, ssq_stft=share1,
                    numpy_second_order=ref['share2'], numpy_first_order=ref['share1'])
    assert abs(share2 - ref['share2']) <= 0.005, (share2, ref['share2'])
    assert share1 < 0.80, share1


# ------------------------------------------------- 4. fallback and thresholds
def _fallback_call(S, dtype, N=1000, n_fft=96, hop=4):
    x, planes, Sfs = five_planes(S, N, n_fft, hop, dtype)
    out = S.ssq_stft2(x, window=gauss(n_fft, 10), n_fft=n_fft, hop_len=hop, fs=FS, dtype=dtype,
                      chirp_tol=np.inf, get_w=True)
    return planes, Sfs, out


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_first_order_fallback(S, dtype):
    """`chirp_tol=inf`: the first-order `w` everywhere -- the definition's for float64; for float32 the value
    `phase_stft` gives (`first_order_float32`), restated here in NumPy -- and `Tx` its ordered reassignment."""
    import torch
    planes, Sfs, (Tx, Sx, ssq_freqs, Sfs2, w) = _fallback_call(S, dtype)
    assert np.array_equal(Sfs, Sfs2)
    assert np.array_equal(_np(Sx), planes[0])
    const = ssq_freqs[1] - ssq_freqs[0]
    assert torch.equal(Tx, S.indexed_sum_onfly(Sx, w, ssq_freqs, const, False, False))
    check_map('stft2_fallback-' + dtype, _np(w), planes, Sfs, default_gamma(dtype), np.inf, np.dtype(dtype),
              fallback32=dtype == 'float32')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_fallback_matches_phase_stft(S, dtype):
    """`chirp_tol=inf`: `w` equals `phase_stft(Sx, dSx, Sfs, gamma)` wherever both are finite, within the
    bound of the map test, ``8 E + spacing(w)``. A point that falls back is given `phase_kernel`'s first-order
    term -- for float32 its float32 numerator and ``|Sx|^2``, the reference's arithmetic, which differs
    from a float64 evaluation of the same stored values by up to two float32 spacings -- so the difference
    is zero for both dtypes."""
    planes, Sfs, (_, _, _, _, w) = _fallback_call(S, dtype)
    gamma = default_gamma(dtype)
    w64, _, _ = statement(*planes, Sfs, gamma, np.inf)
    wld, _, _ = statement(*planes, Sfs, gamma, np.inf, np.clongdouble)
    fin = np.isfinite(w64) & np.isfinite(wld)
    E = float(np.abs(w64 - wld.astype(np.float64))[fin].max())
    w1 = _np(S.phase_stft(planes[0], planes[1], Sfs, gamma))
    wn = _np(w)
    both = np.isfinite(w1) & np.isfinite(wn)
    assert both.any()
    err = np.abs(wn.astype(np.float64) - w1.astype(np.float64))[both]
    bound = (8 * E + np.spacing(w1).astype(np.float64))[both]
    report_measured('stft2_fallback-%s-vs-phase_stft' % dtype, E=E, max_err=float(err.max()),
                    max_err_over_bound=float((err / bound).max()), n_over=int((err > bound).sum()),
                    n=int(both.sum()))
    assert (err <= bound).all(), (float(err.max()), E)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_all_zero_signal(S, dtype):
    import torch
    for x in (np.zeros(300), np.zeros((2, 300))):
        Tx, Sx, _, _, w = S.ssq_stft2(x, n_fft=64, hop_len=3, dtype=dtype, get_w=True)
        assert bool(torch.isinf(w).all()) and bool((w > 0).all())
        assert bool((Tx == 0).all()) and bool((Sx == 0).all())
        assert not bool(torch.isnan(torch.view_as_real(Tx)).any())


# --------------------------------------------------------------- 5. interface
def test_interface(S):
    import torch
    N, n_fft, hop = 400, 64, 2
    x = two_chirps_fs(2 * N)
    kw = dict(n_fft=n_fft, hop_len=hop, fs=FS, dtype='float32')
    xt = torch.as_tensor(x, device=DEV)
    strided = xt[::2]
    assert not strided.is_contiguous()
    ref = S.ssq_stft2(x[::2].copy(), get_w=True, **kw)
    assert len(ref) == 5 and len(S.ssq_stft2(x[::2].copy(), **kw)) == 4
    for other in (S.ssq_stft2(strided, get_w=True, **kw), S.ssq_stft2(strided.contiguous(), get_w=True, **kw)):
        for k in (0, 1, 4):
            assert torch.equal(ref[k], other[k])
        assert np.array_equal(ref[2], other[2]) and np.array_equal(ref[3], other[3])
    host = S.ssq_stft2(x[::2].copy(), get_w=True, astensor=False, **kw)
    for k in (0, 1, 4):
        assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], _np(ref[k]))
    assert isinstance(ref[2], np.ndarray) and isinstance(ref[3], np.ndarray)
    # a batch with get_w, and no gradient whatever x requires
    xb = torch.as_tensor(np.stack([x[:N], x[N:]]), device=DEV, dtype=torch.float32).requires_grad_(True)
    Tb, Sb, _, _, wb = S.ssq_stft2(xb, get_w=True, **kw)
    assert Tb.shape == Sb.shape == wb.shape == (2, n_fft // 2 + 1, (N - 1) // hop + 1)
    assert Tb.grad_fn is None and Sb.grad_fn is None and wb.grad_fn is None
    with pytest.raises(ValueError, match='linearly'):
        S.ssq_stft2(x[:N], ssq_freqs=np.logspace(-2, 0, n_fft // 2 + 1) * FS / 2, **kw)


def test_abi_errors_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert lib.ssq_version() >= 109 and _lib.ABI_VERSION >= 109 and 'ssq_stft2_phase' in _lib.EXPORTS
    rows, n = 4, 6
    planes = [torch.ones((rows, n), dtype=torch.complex64, device=DEV) for _ in range(5)]
    Sfs = torch.linspace(0, .5, rows, dtype=torch.float32, device=DEV)
    w = torch.full((rows, n), 7., dtype=torch.float32, device=DEV)

    def call(ptrs, rows_, n_=n, batch=1, tol=1e-3):
        return lib.ssq_stft2_phase(_lib.F32, *ptrs, Sfs.data_ptr(), w.data_ptr(), batch, rows_, n_, 1e-6, tol, None)

    ptrs = [p.data_ptr() for p in planes]
    for k in range(5):
        bad = list(ptrs)
        bad[k] = None
        assert call(bad, rows) == -1
        assert b'null' in lib.ssq_last_error()
    assert call(ptrs, 1) == -1
    assert b'rows' in lib.ssq_last_error()
    assert call(ptrs, rows, n_=0) == -1 and call(ptrs, rows, batch=0) == -1
    assert call(ptrs, 1 << 16, n_=1 << 8, batch=1 << 8) == -1 and b'2^32' in lib.ssq_last_error()
    assert call(ptrs, rows, tol=-1.) == -1 and call(ptrs, rows, tol=float('nan')) == -1
    assert lib.ssq_stft2_phase(7, *ptrs, Sfs.data_ptr(), w.data_ptr(), 1, rows, n, 1e-6, 1e-3, None) == -1
    if DEV == 'cuda':
        torch.cuda.synchronize()
    assert bool((w == 7).all())
    assert call(ptrs, rows) == 0                # ... and the same arguments, whole, run
    if DEV == 'cuda':
        torch.cuda.synchronize()
    assert not bool((w == 7).any())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_offset_pointers_take_the_element_path(S, dtype, rows=5, n=7):
    """Planes that do not start on a 16-byte boundary (views into a larger buffer) and an odd point
    count: the same bits as the aligned call."""
    import torch
    rng = np.random.default_rng(3)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    planes = [(rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))).astype(cdt) for _ in range(5)]
    Sfs = np.linspace(0, .5, rows).astype(dtype)
    ref = S.phase_stft2_gpu(*planes, Sfs, 1e-3, 1e-3)
    check_map('stft2_map-random-' + dtype, _np(ref), planes, Sfs, 1e-3, 1e-3, np.dtype(dtype))
    if dtype == 'float64':
        return                                  # a complex128 element is 16 bytes: no unaligned view to make
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    bufs = [torch.zeros(rows * n + 1, dtype=torch.complex64, device=DEV) for _ in range(5)]
    for b, p in zip(bufs, planes):
        b[1:] = torch.as_tensor(p.reshape(-1), device=DEV)
    sf = torch.as_tensor(Sfs, device=DEV)
    w = torch.empty(rows * n, dtype=torch.float32, device=DEV)
    ptrs = [b.data_ptr() + 8 for b in bufs]
    assert all(p % 16 == 8 for p in ptrs)
    assert lib.ssq_stft2_phase(_lib.F32, *ptrs, sf.data_ptr(), w.data_ptr(), 1, rows, n, 1e-3, 1e-3, None) == 0
    if DEV == 'cuda':
        torch.cuda.synchronize()
    assert torch.equal(w.reshape(rows, n), ref)


# ------------------------------------------- 6. the parent's bits, the walk
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', second_order.PARENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_parent_bits(S, shape, dtype):
    """`w` on the planes of tests/golden/second_order_parent.npz, bit for bit what the parent commit's library gave
    on the MI355X (recorded by tests/second_order.py)."""
    second_order.assert_parent_bits(S, 'stft', shape, dtype)


@pytest.mark.parametrize('case', ['float32', 'float64', 'float32-offset'])
def test_walk_second_trip(S, case, gamma=1., chirp_tol=.9):
    """More steps than a launch has threads: the whole call against the same entry on blocks of rows
    (`second_order.assert_walk`). `float32-offset`: every plane one element into its buffer, through the raw entry --
    the element path's own second trip. Standard normal planes: `gamma` = 1 makes 39 % of the points `inf`,
    `chirp_tol` = 0.9 splits the rest about evenly."""
    import torch
    from ssqueezepy_amd import _lib
    dtype = case.split('-')[0]
    planes = second_order.walk_planes(dtype, DEV, offset=int(case.endswith('offset')))
    assert all(p.data_ptr() % 16 == (8 if case.endswith('offset') else 0) for p in planes)
    Sfs = np.linspace(0, .5 * FS, second_order.WALK_SHAPE[1]).astype(dtype)

    def raw(planes, Sfs):
        w = torch.empty(planes[0].shape, dtype=planes[0].real.dtype, device=DEV)
        B, rows, n = planes[0].shape if planes[0].ndim == 3 else (1,) + tuple(planes[0].shape)
        sf = torch.as_tensor(Sfs, device=DEV)
        assert _lib.load().ssq_stft2_phase(_lib.F32 if dtype == 'float32' else _lib.F64, *[p.data_ptr() for p in planes], sf.data_ptr(), w.data_ptr(), B,
                                           rows, n, gamma, chirp_tol, None) == 0
        if DEV == 'cuda':
            torch.cuda.synchronize()
        return w

    second_order.assert_walk(raw if case.endswith('offset') else
                             lambda planes, Sfs: S.phase_stft2_gpu(*planes, Sfs, gamma, chirp_tol),
                             planes, Sfs, lambda V, Sfs: V[3] * V[1] - V[4] * V[0], gamma, chirp_tol)
