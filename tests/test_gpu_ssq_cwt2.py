# -*- coding: utf-8 -*-
"""`ssq_cwt2`: the second-order synchrosqueezed CWT (`ssq_cwt2_phase` + the ordered reassignment),
DESIGN.md section 4.5.4.

The oracle of the map is `statement` below: the definition, written in NumPy, evaluated in float64
(the reference) and again in `np.clongdouble`. `E`, the largest difference between the two
evaluations over the finite points, is the reference's own rounding error; the device -- float64
arithmetic per point, products possibly associated otherwise -- must agree with the float64
evaluation to `8 E + spacing(w_ref)` in the output dtype, and on every `inf`. (Where a float32 point
falls back to the first order the definition hands out `phase_cwt`'s value, float32 numerator
included: `first_order_float32`, up to two float32 spacings from a float64 evaluation. For float32
data the reference carries that value at those points -- a handful on the chirps, a quarter of the
synthetic planes; `E` stays that of the float64 definition.) Points within 1e-6 (relative) of one of the two thresholds may fall on either side
and are left out; there may be at most 1e-4 of them.

What the map is *for* is checked on a linear chirp, against a NumPy float64 restatement of the whole
transform (CWTs included): `ssq_cwt2` puts the interior energy into the bin of the true
instantaneous frequency, `ssq_cwt` does not.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import second_order
from second_order import _np, default_gamma, _above_median

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
TWO_PI = 6.283185307179586                 # the float64 constant of the definition
MAP_SHAPES = [(777, 37), (1000, 48), (250, 20)]      # (N, na): n odd -- a 16-byte load straddles two rows
FS = 200.
GMW = dict(gamma=3, beta=60)


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def crossing_chirps(N, seed=0):
    """Two chirps that cross at 0.64 of the record, whatever its length, plus 1e-3 noise; `FS` Hz."""
    t = np.arange(N) / FS
    T = N / FS
    noise = np.random.default_rng(seed).standard_normal(N)
    return (np.cos(2 * np.pi * (10 * t + 30 * t**2 / T)) + .7 * np.cos(2 * np.pi * (80 * t - 25 * t**2 / T))
            + 1e-3 * noise)


def gmw(dtype, **kw):
    from ssqueezepy_amd.wavelets import Wavelet
    return Wavelet(('gmw', dict(GMW, dtype=dtype, **kw)))


def first_order_float32(W, dW):
    """`|w1|` as `phase_cwt` evaluates it for complex64 data, the reference's CPU arithmetic:
    ``Im(dWx conj(Wx))`` and ``|Wx|^2`` in float32, float64 from the 2 pi on."""
    a, b, c, d = dW.real, dW.imag, W.real, W.imag
    assert a.dtype == np.float32
    with np.errstate(all='ignore'):
        num, m2 = b * c - a * d, c * c + d * d
        return np.abs(num.astype(np.float64) / (m2.astype(np.float64) * TWO_PI))


def statement(W, dW, Wd, dWd, dW3, scales, fs, gamma, chirp_tol, ctype=np.complex128, fallback32=False):
    """The definition, operation by operation, in `ctype`. Returns `w` (not yet rounded to an output
    dtype) and the two threshold quantities ``|den| / |W|^2`` and ``|W|``. `fallback32`: the points
    that fall back to the first order carry `phase_cwt`'s value for complex64 data
    (`first_order_float32`), which is what the kernel hands out there."""
    w1_32 = first_order_float32(W, dW) if fallback32 else None
    rtype = np.float64 if ctype == np.complex128 else np.longdouble
    W, dW, Wd, dWd, dW3 = [np.asarray(V).astype(ctype) for V in (W, dW, Wd, dWd, dW3)]
    r = (np.asarray(scales).reshape(-1).astype(rtype) / rtype(fs))[:, None]
    two_pi, j = rtype(TWO_PI), ctype(1j)
    with np.errstate(all='ignore'):
        T, dT, ddW = -j * r * Wd, -j * r * dWd, (j / r) * dW3
        den = W * (W + dT) - T * dW
        num = W * ddW - dW * dW
        w1 = (dW / W).imag / two_pi
        w2 = w1 - (num * T / (den * W)).imag / two_pi
        aW = np.abs(W)
        ratio = np.abs(den) / aW**2
        second = np.abs(den) > rtype(chirp_tol) * aW**2
        w = np.where(second, np.abs(w2), np.abs(w1) if w1_32 is None else w1_32.astype(rtype))
        w = np.where(aW < rtype(gamma), rtype(np.inf), w)
    return w, ratio, aW


def check_map(name, w_dev, planes, scales, fs, gamma, chirp_tol, rdtype, fallback32=False):
    """`second_order.check_map` on this module's `statement`; with `fallback32` the reference carries
    `phase_cwt`'s float32 first-order value at the points that fall back."""
    ref = statement(*planes, scales, fs, gamma, chirp_tol, fallback32=True)[0] if fallback32 else None
    return second_order.check_map(name, w_dev, statement(*planes, scales, fs, gamma, chirp_tol),
                                  statement(*planes, scales, fs, gamma, chirp_tol, np.clongdouble), gamma, chirp_tol,
                                  rdtype, ref)


def log_scales(N, na, dtype):
    """`na` log-spaced scales (in samples) from the GMW's peak at 0.29 cycles per sample down to 8 periods
    of the record, in the wavelet's dtype as the design step hands them to the plans."""
    return np.geomspace(1.5, N / 8, na).astype(dtype)


_PLANES = {}


def three_plans(wavelet, scales, N, batch, dt):
    from ssqueezepy_amd._cwt import get_cwt_plan
    from ssqueezepy_amd.wavelets import derived_wavelets
    return [get_cwt_plan(wv, scales, N, 'reflect', dt, True, batch)
            for wv in (wavelet,) + tuple(derived_wavelets(wavelet))]


def five_planes(S, N, na, dtype, batch=None):
    """The five planes of the test signal (host arrays) from the package's own CWT plans over the banks
    `ssq_cwt2` uses; computed once per configuration and shared; nobody writes to them."""
    key = (N, na, dtype, batch)
    if key not in _PLANES:
        import torch
        x = (crossing_chirps(N) if batch is None else
             np.stack([crossing_chirps(N, seed=s) * (1 + s) for s in range(batch)]))
        scales = log_scales(N, na, dtype)
        xd = torch.as_tensor(x.astype(dtype), device=DEV)
        outs = [p.execute(xd, want_dWx=True)
                for p in three_plans(gmw(dtype), scales, N, 1 if batch is None else batch, 1 / FS)]
        planes = tuple(_np(p) for p in (outs[0]['Wx'], outs[0]['dWx'], outs[1]['Wx'], outs[1]['dWx'],
                                        outs[2]['dWx']))
        _PLANES[key] = (x, planes, scales)
    return _PLANES[key]


# ---------------------------------------------------------------- 1. the map
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', MAP_SHAPES + [(250, 20, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_map_vs_numpy_statement(S, shape, dtype):
    N, na = shape[:2]
    batch = shape[2] if len(shape) == 3 else None
    _, planes, scales = five_planes(S, N, na, dtype, batch)
    gamma = default_gamma(dtype)
    w = S.phase_cwt2_gpu(*planes, scales, FS, gamma, 1e-3)
    assert tuple(w.shape) == planes[0].shape and str(w.dtype).endswith(dtype)
    name = 'cwt2_map-%s-%s' % ('x'.join(map(str, shape)), dtype)
    if batch is None:
        check_map(name, _np(w), planes, scales, FS, gamma, 1e-3, np.dtype(dtype), fallback32=dtype == 'float32')
    else:
        for b in range(batch):
            check_map('%s[%d]' % (name, b), _np(w)[b], [p[b] for p in planes], scales, FS, gamma, 1e-3,
                      np.dtype(dtype), fallback32=dtype == 'float32')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', [(3, 5, 7), (1, 33, 129)], ids=lambda s: 'x'.join(map(str, s)))
def test_map_on_random_planes_takes_all_three_branches(S, shape, dtype):
    """Synthetic planes with `gamma` at the median ``|W|`` and `chirp_tol` at the median ``|den| / |W|^2``
    of the points above it: a half is `inf`, the rest splits between the second order and the fallback."""
    rng = np.random.default_rng(11)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    planes = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt) for _ in range(5)]
    B, na, n = shape
    scales = np.geomspace(2, 40, na).astype(dtype)
    flat = [p.reshape(B * na, n) for p in planes]
    rows = np.tile(scales, B)                               # the statement's rows: (batch, na) flattened
    _, ratio, aW = statement(*flat, rows, FS, 0., 0.)
    gamma = _above_median(aW)
    tol = _above_median(ratio[aW > gamma])
    w = S.phase_cwt2_gpu(*planes, scales, FS, gamma, tol)
    assert tuple(w.shape) == shape
    name = 'cwt2_map-random-%s-%s' % ('x'.join(map(str, shape)), dtype)
    check_map(name, _np(w).reshape(B * na, n), flat, rows, FS, gamma, tol, np.dtype(dtype),
              fallback32=dtype == 'float32')
    w_ref, ratio, aW = statement(*flat, rows, FS, gamma, tol)
    n_inf, n_2 = int(np.isinf(w_ref).sum()), int(((ratio > tol) & (aW >= gamma)).sum())
    n_1 = w_ref.size - n_inf - n_2
    assert min(n_inf, n_2 + n_1) >= .45 * w_ref.size and min(n_1, n_2) >= .2 * w_ref.size, (n_inf, n_2, n_1)


# ------------------------------------------------------- 2. chirp_tol = inf
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_infinite_chirp_tol_is_phase_cwt(S, dtype, N=250, na=20):
    """`chirp_tol=inf`: `phase_cwt_gpu(Wx, dWx, gamma)` bit for bit, infinities included -- on the planes
    of the map test, on random planes around a `gamma` that cuts them in half, and through `ssq_cwt2`."""
    import torch
    x, planes, scales = five_planes(S, N, na, dtype)
    for gamma in (default_gamma(dtype), float(np.median(np.abs(planes[0])))):
        w = S.phase_cwt2_gpu(*planes, scales, FS, gamma, np.inf)
        w1 = S.phase_cwt_gpu(planes[0], planes[1], gamma)
        assert torch.equal(w, w1)
        assert bool(torch.isfinite(w).any())
    assert bool(torch.isinf(w).any())                       # the median cut: both kinds of point were compared
    wav = gmw(dtype)
    Tx, Wx, _, sc, w = S.ssq_cwt2(x, wav, fs=FS, nv=8, chirp_tol=np.inf, get_w=True)
    dWx = three_plans(wav, sc, N, 1, 1 / FS)[0].execute(torch.as_tensor(x.astype(dtype), device=DEV),
                                                        want_dWx=True)['dWx']
    assert torch.equal(w, S.phase_cwt_gpu(Wx, dWx, default_gamma(dtype)))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_impulse_falls_back(S, dtype, N=400):
    """An impulse has no chirp rate: ``den / W^2`` is 0 up to rounding (a NumPy float64 restatement gave
    1.6e-15, the float32 planes here 1e-5), so around the impulse `w` is the first-order one, bit for bit.
    "Around": where ``|W|`` is within a factor 10 of its row's largest, on the rows that see one impulse --
    scales from 1.5 samples (the wavelet's band clear of Nyquist) to N / 50 (the record's reflection puts
    the next impulse N samples away, and a GMW(3, 60) at scale a has a standard deviation of 4.9 a samples:
    at 10 deviations its tail is e^-50)."""
    import torch
    x = np.zeros(N)
    x[N // 2] = 1.
    wav = gmw(dtype)
    Tx, Wx, _, sc, w = S.ssq_cwt2(x, wav, fs=FS, nv=8, get_w=True)
    dWx = three_plans(wav, sc, N, 1, 1 / FS)[0].execute(torch.as_tensor(x.astype(dtype), device=DEV),
                                                        want_dWx=True)['dWx']
    w1 = _np(S.phase_cwt_gpu(Wx, dWx, default_gamma(dtype)))
    aW = np.abs(_np(Wx))
    rows = (sc >= 1.5) & (sc <= N / 50)
    strong = (aW >= .1 * aW.max(axis=1, keepdims=True)) & rows[:, None]
    same = _np(w) == w1
    report_measured('cwt2_impulse-' + dtype, rows=int(rows.sum()), n_strong=int(strong.sum()),
                    fell_back=int((same & strong).sum()))
    assert rows.sum() >= 8 and strong.sum() >= 3 * rows.sum()
    assert same[strong].all()
    assert np.isfinite(w1[strong]).all()


# ------------------------------------------ 3. the three plans vs a dense FFT
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('N', [1000, 4096])
def test_three_plans_vs_dense_fft(S, N, dtype):
    """`Wx`, `dWx` of the three plans against ``ifft(bank * fft(pad x))`` in NumPy float64 with each plan's
    own `dense_bank` (the derived banks change sign and are user functions to the plan: no float64 twin,
    no continuation past Nyquist for float32). The project's norms: 1e-5 (float32) / 1e-12 (float64) of the
    plane's largest magnitude."""
    import torch
    from ssqueezepy_amd.scales import process_scales
    wav = gmw(dtype)
    scales = np.asarray(process_scales('log', N, wav, nv=8), dtype=dtype).reshape(-1)
    x = crossing_chirps(N).astype(dtype)
    xd = torch.as_tensor(x, device=DEV)
    tol = 1e-5 if dtype == 'float32' else 1e-12
    for name, plan in zip(('psih', 'dpsih', 'w_psih'), three_plans(wav, scales, N, 1, 1 / FS)):
        out = plan.execute(xd, want_dWx=True)
        P = _np(plan.dense_bank(xd.device)).astype(np.float64)
        src = _np(plan.pad_sources(xd.device))
        xh = np.fft.fft(x.astype(np.float64)[src])
        k = np.arange(plan.M)
        xi = np.where(k <= plan.M // 2, k, k - plan.M) * (2 * np.pi / plan.M)
        sl = slice(plan.n1, plan.n1 + N)
        refs = {'Wx': np.fft.ifft(P * xh)[:, sl], 'dWx': np.fft.ifft(P * xh * (1j * xi * FS))[:, sl]}
        errs = {}
        for k_, ref in refs.items():
            errs[k_] = float(np.abs(_np(out[k_]) - ref).max() / np.abs(ref).max())
        report_measured('cwt2_plan-%s-%d-%s' % (name, N, dtype), algo=plan.algo, block_rows=plan.block_rows,
                        na=plan.na, **errs)
        assert max(errs.values()) <= tol, (name, errs)


# ------------------------------------------------- 4. Tx = ordered reassignment
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('flipud', [False, True])
@pytest.mark.parametrize('ssq_freqs', [None, 'linear'])
def test_tx_is_ordered_reassignment_of_w(S, dtype, flipud, ssq_freqs, N=500, nv=8, B=3):
    import torch
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    from ssqueezepy_amd.ssqueezing import GRID_LIN
    wav = gmw(dtype)
    xb = np.stack([crossing_chirps(N, seed=s) * (1 + s) for s in range(B)])
    kw = dict(fs=FS, nv=nv, ssq_freqs=ssq_freqs, flipud=flipud)
    scales_dt, grid_freqs, const, grid, _ = _ssq_design(wav, 'log-piecewise', nv, N, 1 / FS, ssq_freqs, 'peak', True)
    singles = []
    for x in (xb[1], xb):
        Tx, Wx, freqs, scales, w = S.ssq_cwt2(x, wav, get_w=True, **kw)
        na = len(scales)
        assert Tx.shape == Wx.shape == w.shape == x.shape[:-1] + (na, N)
        assert Tx.grad_fn is None and Wx.grad_fn is None and w.grad_fn is None
        assert np.array_equal(freqs, grid_freqs[::-1]) and np.array_equal(scales, scales_dt.squeeze())
        assert torch.equal(Tx, S.indexed_sum_onfly(Wx, w, grid_freqs, const, grid != GRID_LIN, flipud))
        again = S.ssq_cwt2(x, wav, get_w=True, **kw)
        assert torch.equal(Tx, again[0]) and torch.equal(w, again[4]) and torch.equal(Wx, again[1])
        xd = torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)
        plan = three_plans(wav, scales_dt, N, x.shape[0] if x.ndim == 2 else 1, 1 / FS)[0]
        assert torch.equal(Wx, plan.execute(xd, want_dWx=True)['Wx'])
        assert len(S.ssq_cwt2(x, wav, **kw)) == 4
        singles.append((Tx, Wx, w))
    (T1, W1, w1), (Tb, Wb, wb) = singles
    assert torch.equal(Tb[1], T1) and torch.equal(Wb[1], W1) and torch.equal(wb[1], w1)
    assert float(torch.abs(T1).max()) > 0


# ------------------------------------------------------- 5. what it is for
CHIRP = dict(N=1024, rate=3e-4, f0=.03, nv=32)


def np_cwt(x, fn, scales, M, n1, deriv, dtype):
    """``ifft(fn(a xi) fft(pad x))`` (times ``1j xi`` for the time derivative, fs = 1), reflect padding to
    `M`, with everything in `dtype`: the bank, the signal, and the transforms themselves (scipy.fft computes
    float32 input in float32), so that the float32 restatement differs from the float64 one by what float32
    does to a whole transform, not to its result only."""
    import scipy.fft
    N = len(x)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    xp = np.pad(np.asarray(x, dtype=dtype), (n1, M - N - n1), mode='reflect')
    k = np.arange(M)
    xi = (np.where(k <= M // 2, k, k - M) * (2 * np.pi / M)).astype(dtype)
    with np.errstate(all='ignore'):
        P = np.asarray(fn(np.asarray(scales, dtype=dtype).reshape(-1, 1) * xi)).astype(dtype)
    P[:, M // 2] /= 2
    xh = scipy.fft.fft(xp.astype(cdt))
    if deriv:
        xh = xh * (1j * xi).astype(cdt)
    out = scipy.fft.ifft(P * xh, axis=-1)[:, n1:n1 + N]
    assert out.dtype == cdt
    return out


def np_reassign(Wx, w, ssq_freqs, const):
    """`indexed_sum_onfly` on a log grid, in NumPy (sums in float64, ascending rows)."""
    l0 = np.log2(ssq_freqs[0])
    dl = np.log2(ssq_freqs[1]) - l0
    Tx = np.zeros(Wx.shape, dtype=np.complex128)
    ok = np.isfinite(w) & (w > 0)
    with np.errstate(all='ignore'):
        k = np.clip(np.rint((np.log2(np.where(ok, w, 1.).astype(np.float64)) - l0) / dl), 0, len(ssq_freqs) - 1)
    k = k.astype(int)
    for i in range(Wx.shape[0]):
        cols = np.nonzero(ok[i])[0]
        np.add.at(Tx, (k[i, cols], cols), Wx[i, cols].astype(np.complex128) * const)
    return Tx


def ridge_share(Tx, bins, cols):
    E = np.abs(Tx[:, cols])**2
    return float(E[bins[cols], np.arange(len(cols))].sum() / E.sum())


_CHIRP = {}


def chirp_reference():
    """The chirp of the issue on the product's own scale design, and the NumPy restatement of both
    transforms on it in float64 and in float32 (banks and planes in that type, the map as defined): the
    shares of the interior energy in the bin of the true instantaneous frequency. Computed once."""
    if not _CHIRP:
        from ssqueezepy_amd._ssq_cwt import _ssq_design
        from ssqueezepy_amd.padding import pad_geometry
        from ssqueezepy_amd.wavelets import derived_wavelets
        N, rate, f0, nv = CHIRP['N'], CHIRP['rate'], CHIRP['f0'], CHIRP['nv']
        n = np.arange(N)
        x = np.cos(2 * np.pi * (f0 * n + .5 * rate * n**2))
        M, n1, _ = pad_geometry(N)
        shares = {}
        for dtype in ('float64', 'float32'):
            wav = gmw(dtype)
            scales, freqs, const, _, _ = _ssq_design(wav, 'log', nv, N, 1., None, 'peak', True)
            scales = scales.reshape(-1)
            d, wp = derived_wavelets(wav)
            V = [np_cwt(x, fn, scales, M, n1, deriv, dtype)
                 for fn, deriv in ((wav.fn, 0), (wav.fn, 1), (d.fn, 0), (d.fn, 1), (wp.fn, 1))]
            gamma = default_gamma(dtype)
            f32 = dtype == 'float32'
            w2 = statement(*V, scales, 1., gamma, 1e-3, fallback32=f32)[0].astype(dtype)
            w1 = statement(*V, scales, 1., gamma, np.inf, fallback32=f32)[0].astype(dtype)
            bins = np.rint((np.log2(f0 + rate * n) - np.log2(freqs[0])) / (np.log2(freqs[1]) - np.log2(freqs[0])))
            bins = np.clip(bins, 0, len(freqs) - 1).astype(int)
            cols = np.arange(N // 4, N - N // 4)
            shares[dtype] = (ridge_share(np_reassign(V[0], w2, freqs, const), bins, cols),
                             ridge_share(np_reassign(V[0], w1, freqs, const), bins, cols))
        _CHIRP.update(x=x, bins=bins, cols=cols, shares=shares,
                      margin2=4 * abs(shares['float32'][0] - shares['float64'][0]),
                      margin1=4 * abs(shares['float32'][1] - shares['float64'][1]))
    return _CHIRP


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_sharpens_a_linear_chirp(S, dtype):
    """Device shares against the restatement's of the same dtype, within 4 x the restatement's own
    float32-versus-float64 difference (the only yardstick of what rounding does to a share that does not
    come from the code under test).

    Which float32 restatement: the one whose transforms run in float32 (`np_cwt`, scipy.fft on complex64).
    A restatement that transforms in float64 and only rounds the finished planes to complex64 is the other
    reading; it leaves each point a relative error of 6e-8, where any float32 transform -- pocketfft's as
    much as the device's -- leaves an error of that order relative to the plane's LARGEST value, i.e. far
    more on a ridge's skirts, which is where energy leaves the bin. Figures, second order: float64
    restatement 0.9999983; float32, planes rounded only 0.9999973 (margin 3.8e-6); float32, float32
    transforms 0.9999911 (margin 2.9e-5); MI355X float32 0.9999925, float64 0.9999983. Measured against
    the rounded-planes reading the device's float32 share is off by 4.8e-6 and misses its margin by 1.1e-6;
    against the float32-transform reading it is off by 1.4e-6 of 2.9e-5 allowed. The second reading is the
    one that measures what the test is after, so it is the oracle; the first order is hardly sensitive to
    the choice (margins 2.5e-6 and 3.7e-6, device within 4e-7 of either)."""
    ref = chirp_reference()
    share2_ref, share1_ref = ref['shares'][dtype]
    # the oracle itself: the signal was chosen so that the float64 restatement alone separates the two
    assert ref['shares']['float64'][0] >= 0.999 and ref['shares']['float64'][1] <= 0.95, ref['shares']
    kw = dict(scales='log', nv=CHIRP['nv'], fs=1., flipud=False)
    wav = gmw(dtype)
    share2 = ridge_share(_np(S.ssq_cwt2(ref['x'], wav, **kw)[0]), ref['bins'], ref['cols'])
    share1 = ridge_share(_np(S.ssq_cwt(ref['x'], wav, **kw)[0]), ref['bins'], ref['cols'])
    report_measured('cwt2_chirp_share-' + dtype, ssq_cwt2=share2, ssq_cwt=share1, numpy_second_order=share2_ref,
                    numpy_first_order=share1_ref, margin_second_order=ref['margin2'],
                    margin_first_order=ref['margin1'])
    assert abs(share2 - share2_ref) <= ref['margin2'], (share2, share2_ref, ref['margin2'])
    assert abs(share1 - share1_ref) <= ref['margin1'], (share1, share1_ref, ref['margin1'])


# ------------------------------------------------ 6. zero signal, ABI, offsets
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_all_zero_signal(S, dtype):
    import torch
    wav = gmw(dtype)
    for x in (np.zeros(300), np.zeros((2, 300))):
        Tx, Wx, _, _, w = S.ssq_cwt2(x, wav, nv=8, get_w=True)
        assert bool(torch.isinf(w).all()) and bool((w > 0).all())
        assert bool((Tx == 0).all()) and bool((Wx == 0).all())
        assert not bool(torch.isnan(torch.view_as_real(Tx)).any())


def test_interface(S):
    import torch
    N = 300
    x = crossing_chirps(2 * N)
    kw = dict(fs=FS, nv=8)
    xt = torch.as_tensor(x, device=DEV)
    strided = xt[::2]
    assert not strided.is_contiguous()
    ref = S.ssq_cwt2(x[::2].copy(), get_w=True, **kw)                # the default wavelet, float32
    assert len(ref) == 5 and ref[0].dtype == torch.complex64 and ref[4].dtype == torch.float32
    other = S.ssq_cwt2(strided, get_w=True, **kw)
    for k in (0, 1, 4):
        assert torch.equal(ref[k], other[k])
    assert np.array_equal(ref[2], other[2]) and np.array_equal(ref[3], other[3])
    host = S.ssq_cwt2(x[::2].copy(), get_w=True, astensor=False, **kw)
    for k in (0, 1, 4):
        assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], _np(ref[k]))
    xb = torch.as_tensor(np.stack([x[:N], x[N:]]), device=DEV, dtype=torch.float32).requires_grad_(True)
    Tb, Wb, _, _, wb = S.ssq_cwt2(xb, get_w=True, **kw)
    assert Tb.shape == Wb.shape == wb.shape and Tb.shape[0] == 2
    assert Tb.grad_fn is None and Wb.grad_fn is None and wb.grad_fn is None
    out = S.ssq_cwt2(x[:N], ('morlet', {'mu': 6.}), **kw)            # the other family with a closed form
    assert bool(torch.isfinite(torch.view_as_real(out[0])).all()) and float(torch.abs(out[0]).max()) > 0
    for bad in ('bump', ('gmw', {'order': 1}), lambda w: np.exp(-(w - 5)**2)):
        with pytest.raises(NotImplementedError, match='morlet'):
            S.ssq_cwt2(x[:N], bad, **kw)


def test_abi_errors_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert lib.ssq_version() >= 110 and _lib.ABI_VERSION >= 110 and 'ssq_cwt2_phase' in _lib.EXPORTS
    na, n = 4, 6
    planes = [torch.ones((na, n), dtype=torch.complex64, device=DEV) for _ in range(5)]
    good = np.array([2., 4., 8., 16.])
    w = torch.full((na, n), 7., dtype=torch.float32, device=DEV)

    def call(ptrs, na_=na, n_=n, batch=1, tol=1e-3, fs=FS, scales=good, dtype=_lib.F32):
        sc = np.ascontiguousarray(scales, dtype=np.float64)
        return lib.ssq_cwt2_phase(dtype, *ptrs, sc.ctypes.data if sc.size else None, w.data_ptr(), batch, na_, n_,
                                  fs, 1e-6, tol, None)

    ptrs = [p.data_ptr() for p in planes]
    for k in range(5):
        bad = list(ptrs)
        bad[k] = None
        assert call(bad) == -1 and b'null' in lib.ssq_last_error()
    assert call(ptrs, scales=np.zeros(0)) == -1 and b'null' in lib.ssq_last_error()
    assert call(ptrs, na_=0) == -1 and call(ptrs, n_=0) == -1 and call(ptrs, batch=0) == -1
    assert b'shape' in lib.ssq_last_error()
    assert call(ptrs, 1 << 16, n_=1 << 8, batch=1 << 8) == -1 and b'2^32' in lib.ssq_last_error()
    assert call(ptrs, tol=-1.) == -1 and call(ptrs, tol=float('nan')) == -1 and b'chirp_tol' in lib.ssq_last_error()
    for fs in (0., -1., float('nan'), float('inf')):
        assert call(ptrs, fs=fs) == -1 and b'fs' in lib.ssq_last_error()
    for s in (0., -2., float('nan'), float('inf')):
        bad = good.copy()
        bad[2] = s
        assert call(ptrs, scales=bad) == -1 and b'scales[2]' in lib.ssq_last_error()
    assert call(ptrs, dtype=7) == -1
    if DEV == 'cuda':
        torch.cuda.synchronize()
    assert bool((w == 7).all())
    assert call(ptrs) == 0                      # ... and the same arguments, whole, run
    if DEV == 'cuda':
        torch.cuda.synchronize()
    assert not bool((w == 7).any())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_offset_pointers_take_the_element_path(S, dtype, na=5, n=7):
    """Planes that do not start on a 16-byte boundary (views into a larger buffer) and an odd point
    count: the same bits as the aligned call."""
    import torch
    rng = np.random.default_rng(3)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    planes = [(rng.standard_normal((na, n)) + 1j * rng.standard_normal((na, n))).astype(cdt) for _ in range(5)]
    scales = np.geomspace(2, 30, na)
    ref = S.phase_cwt2_gpu(*planes, scales, FS, .5, .5)
    assert bool(torch.isinf(ref).any()) and bool(torch.isfinite(ref).any())
    if dtype == 'float64':
        return                                  # a complex128 element is 16 bytes: no unaligned view to make
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    bufs = [torch.zeros(na * n + 1, dtype=torch.complex64, device=DEV) for _ in range(5)]
    for b, p in zip(bufs, planes):
        b[1:] = torch.as_tensor(p.reshape(-1), device=DEV)
    ptrs = [b.data_ptr() + 8 for b in bufs]
    assert all(p % 16 == 8 for p in ptrs)
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    for off in (0, 1):                          # w itself on and off an 8-byte boundary
        wbuf = torch.empty(na * n + 1, dtype=torch.float32, device=DEV)
        assert lib.ssq_cwt2_phase(_lib.F32, *ptrs, sc.ctypes.data, wbuf.data_ptr() + 4 * off, 1, na, n, FS, .5, .5,
                                  None) == 0
        if DEV == 'cuda':
            torch.cuda.synchronize()
        assert torch.equal(wbuf[off:off + na * n].reshape(na, n), ref)
    # aligned planes, w off its 8-byte boundary: the element path again
    al = [torch.as_tensor(p, device=DEV) for p in planes]
    wbuf = torch.empty(na * n + 1, dtype=torch.float32, device=DEV)
    assert lib.ssq_cwt2_phase(_lib.F32, *[a.data_ptr() for a in al], sc.ctypes.data, wbuf.data_ptr() + 4, 1, na, n,
                              FS, .5, .5, None) == 0
    if DEV == 'cuda':
        torch.cuda.synchronize()
    assert torch.equal(wbuf[1:].reshape(na, n), ref)


# ------------------------------------------- 7. the parent's bits, the walk
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', second_order.PARENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_parent_bits(S, shape, dtype):
    """`w` on the planes of tests/golden/second_order_parent.npz, bit for bit what the parent commit's library gave
    on the MI355X (recorded by tests/second_order.py)."""
    second_order.assert_parent_bits(S, 'cwt', shape, dtype)


@pytest.mark.parametrize('case', ['float32', 'float64', 'float32-offset'])
def test_walk_second_trip(S, case, gamma=1., chirp_tol=1.):
    """More steps than a launch has threads: the whole call against the same entry on blocks of rows
    (`second_order.assert_walk`). `float32-offset`: every plane one element into its buffer, through the raw entry --
    the element path's own second trip. Standard normal planes: `gamma` = 1 makes 39 % of the points `inf`; with
    ``r = scales / fs`` <= 0.2, ``|den| / |W|^2`` scatters around 1, and `chirp_tol` = 1 splits the rest about evenly."""
    import torch
    from ssqueezepy_amd import _lib
    dtype = case.split('-')[0]
    planes = second_order.walk_planes(dtype, DEV, offset=int(case.endswith('offset')))
    assert all(p.data_ptr() % 16 == (8 if case.endswith('offset') else 0) for p in planes)
    scales = np.geomspace(2, 40, second_order.WALK_SHAPE[1])

    def raw(planes, scales):
        w = torch.empty(planes[0].shape, dtype=planes[0].real.dtype, device=DEV)
        B, na, n = planes[0].shape if planes[0].ndim == 3 else (1,) + tuple(planes[0].shape)
        sc = np.ascontiguousarray(scales, dtype=np.float64)
        assert _lib.load().ssq_cwt2_phase(_lib.F32 if dtype == 'float32' else _lib.F64, *[p.data_ptr() for p in planes], sc.ctypes.data, w.data_ptr(), B,
                                          na, n, FS, gamma, chirp_tol, None) == 0
        if DEV == 'cuda':
            torch.cuda.synchronize()
        return w

    def den(V, scales):
        r = torch.as_tensor(scales / FS, dtype=V[0].real.dtype, device=DEV)[:, None]
        return V[0] * (V[0] - 1j * r * V[3]) + 1j * r * V[2] * V[1]

    second_order.assert_walk(raw if case.endswith('offset') else
                             lambda planes, scales: S.phase_cwt2_gpu(*planes, scales, FS, gamma, chirp_tol),
                             planes, scales, den, gamma, chirp_tol)
