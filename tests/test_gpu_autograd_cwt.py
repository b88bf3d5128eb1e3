# -*- coding: utf-8 -*-
"""The backward of the CWT plan (`ssq_cwt_adjoint` through `CwtPlan.adjoint`): gradients of `cwt`
through `Wx` AND `dWx`, and of `ssq_cwt`, for whole batches in one call.

The plan's map is linear in `x`:  Wx_a = unpad ifft(psih_a fft(pad x)),  dWx_a = the same with
psih_a (1j m_k), m_k the forward's derivative multiplier xi_k / dt rounded as the kernels round it.
Its adjoint is checked against the closed form

    gx = pad^T Re ifft( sum_a psih_a (fft(U gW_a) - 1j m_k fft(U gdW_a)) )

evaluated in float64 from `plan.dense_bank` and `plan.pad_sources` (called after the adjoint: the
adjoint itself must need neither), against torch.autograd through a float64 torch statement of the
forward, and against the plan's own forward through <A x, g> = <x, A^H g>.

Tolerances: the suite's 1e-5 (float32) / 1e-12 (float64) of the largest magnitude for a transform,
20 x that for an adjoint (the margin of test_cwt_is_differentiable and test_gpu_autograd.py).
"""
import ctypes
import os
import numpy as np
import pytest
from conftest import two_chirps

pytestmark = pytest.mark.gpu
TOL = {'float32': 1e-5, 'float64': 1e-12}
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
BUDGET = 2 << 30          # the plan's product workspace budget (csrc/ssq_cwt.hip: ssq_cwt_plan_create)


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _tdt(dtype, cplx=False):
    import torch
    return {('float32', False): torch.float32, ('float64', False): torch.float64,
            ('float32', True): torch.complex64, ('float64', True): torch.complex128}[(dtype, cplx)]


def _wavelet(S, dtype, l1_norm):
    return S.Wavelet(('gmw' if l1_norm else 'morlet', {'dtype': dtype}))


def _plan(S, dtype, N, padtype, l1_norm=True, fs=1., max_batch=1, nv=8, scales='log-piecewise'):
    """A fresh (uncached) plan as `cwt` would make it."""
    from ssqueezepy_amd import _cwt
    wav = _wavelet(S, dtype, l1_norm)
    if isinstance(scales, str):
        scales = S.process_scales(scales, N, wav, nv=nv)
    scales = np.asarray(scales, dtype=dtype)
    return _cwt.get_cwt_plan(wav, scales, N, padtype, 1. / fs, l1_norm, max_batch, cache=False)


def _multiplier(plan):
    """m_k as bank_multiply_kernel forms it: (T)(ks * 2 pi / M) * (T(1) / T(dt)), as float64."""
    rdt = np.dtype(plan.dtype).type
    k = np.arange(plan.M)
    ks = np.where(k <= plan.M // 2, k, k - plan.M).astype(np.float64)
    h = (2.0 * 3.141592653589793) / float(plan.M)
    return ((ks * h).astype(rdt) * (rdt(1) / rdt(plan.dt))).astype(np.float64)


def closed_form(plan, gW, gdW, rpadded, dev):
    """The adjoint's formula in float64 (NumPy) for one signal; gW / gdW: (na, cols) or None."""
    psih = _np(plan.dense_bank(dev)).astype(np.float64)
    src = _np(plan.pad_sources(dev))
    M, N, n1 = plan.M, plan.N, plan.n1

    def spectrum(g):
        G = np.zeros((plan.na, M), dtype=np.complex128)
        if rpadded:
            G[:] = g
        else:
            G[:, n1:n1 + N] = g
        return np.fft.fft(G, axis=-1)

    spec = np.zeros((plan.na, M), dtype=np.complex128)
    if gW is not None:
        spec += spectrum(gW)
    if gdW is not None:
        spec -= 1j * _multiplier(plan)[None] * spectrum(gdW)
    y = np.fft.ifft((psih * spec).sum(0)).real
    gx = np.zeros(N)
    np.add.at(gx, src[src >= 0], y[src >= 0])
    return gx


def torch_cwt(plan, x, rpadded=False):
    """The plan's forward as torch ops on a float64 `x` (differentiable): pad gather, fft, bank,
    the 1j m_k multiplier, ifft, slice. Returns Wx, dWx."""
    import torch
    dev = x.device
    psih = plan.dense_bank(dev).to(torch.float64)
    src = plan.pad_sources(dev)
    m = torch.as_tensor(_multiplier(plan), device=dev)
    xp = torch.where(src >= 0, x[..., src.clamp(min=0)], torch.zeros((), dtype=x.dtype, device=dev))
    xh = torch.fft.fft(xp, dim=-1)[..., None, :]
    W = torch.fft.ifft(psih * xh, dim=-1)
    dW = torch.fft.ifft(psih * (1j * m) * xh, dim=-1)
    if not rpadded:
        W, dW = W[..., plan.n1:plan.n1 + plan.N], dW[..., plan.n1:plan.n1 + plan.N]
    return W, dW


def _loss(Wx, dWx, wgt, wgt2):
    """A loss over both outputs, of the form of `_stft_loss` in test_gpu_autograd.py."""
    import torch
    loss = (torch.abs(Wx)**2 * wgt).sum() + (Wx.real * wgt).sum()
    if dWx is not None:
        loss = loss + (torch.abs(dWx)**2 * wgt2).sum() + (dWx.imag * wgt2).sum()
    return loss


def _random_c(rng, shape, dtype):
    import torch
    return torch.as_tensor(rng.standard_normal(shape) + 1j * rng.standard_normal(shape),
                           dtype=_tdt(dtype, True), device=DEV)


# (dtype, padtype, l1_norm, N, fs, B [0: 1-D], rpadded)
ADJOINT_CASES = [
    ('float32', 'reflect', True, 300, 1., 3, False),
    ('float64', 'reflect', True, 300, 1., 0, False),
    ('float32', 'zero', True, 301, 1., 1, False),                # an odd N
    ('float64', 'symmetric', False, 300, 1., 3, False),          # row_scale
    ('float32', 'replicate', False, 300, 4., 0, False),          # fs != 1, row_scale
    ('float32', 'wrap', True, 257, 1., 1, False),
    ('float32', None, True, 300, 1., 3, False),                  # no padding: M = N, not a power of two
    ('float32', None, True, 301, 2., 0, False),                  # ... and odd: the 8-byte path of the float32 kernels
    ('float64', None, False, 301, 1., 1, False),
    ('float32', 'reflect', True, 300, 1., 3, True),              # gradients of padded width
    ('float64', 'zero', True, 301, .5, 0, True),
]


@pytest.mark.parametrize('case', ADJOINT_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_cwt_adjoint_vs_closed_form(S, case):
    """`plan.adjoint(gW, gdW)` with `gW` only, `gdW` only and both against the closed form."""
    dtype, padtype, l1_norm, N, fs, B, rpadded = case
    rng = np.random.default_rng(N + B)
    plan = _plan(S, dtype, N, padtype, l1_norm, fs, max_batch=max(B, 1))
    cols = plan.M if rpadded else N
    shape = ((B,) if B else ()) + (plan.na, cols)
    gW, gdW = _random_c(rng, shape, dtype), _random_c(rng, shape, dtype)
    outs = [plan.adjoint(gW, None, rpadded=rpadded), plan.adjoint(None, gdW, rpadded=rpadded),
            plan.adjoint(gW, gdW, rpadded=rpadded)]
    assert plan._psih_dev is None, "the adjoint built a dense bank"
    for out, (a, d) in zip(outs, ((gW, None), (None, gdW), (gW, gdW))):
        assert tuple(out.shape) == ((B,) if B else ()) + (N,)
        assert out.dtype == _tdt(dtype)
        nb = max(B, 1)
        a3 = None if a is None else _np(a).reshape(nb, plan.na, cols)
        d3 = None if d is None else _np(d).reshape(nb, plan.na, cols)
        o3 = _np(out).reshape(nb, N)
        want = np.stack([closed_form(plan, None if a3 is None else a3[b], None if d3 is None else d3[b],
                                     rpadded, out.device) for b in range(nb)])
        err = relmax(o3.astype(np.float64), want)
        print("measured: cwt adjoint", case, a is not None, d is not None, err)
        assert err <= 20 * TOL[dtype]


def test_cwt_adjoint_argument_errors(S):
    """Shape mismatch, both None and B > max_batch raise ValueError; a conjugated view and a wider
    dtype are resolved as `StftPlan.adjoint` resolves them."""
    import torch
    plan = _plan(S, 'float32', 300, 'reflect', max_batch=2)
    rng = np.random.default_rng(0)
    g = _random_c(rng, (2, plan.na, 300), 'float32')
    with pytest.raises(ValueError):
        plan.adjoint(None, None)
    with pytest.raises(ValueError):
        plan.adjoint(g[:, :, :-1])
    with pytest.raises(ValueError):
        plan.adjoint(g, g[0])
    with pytest.raises(ValueError):
        plan.adjoint(torch.cat([g, g]))
    with pytest.raises(ValueError):
        plan.adjoint(g, rpadded=True)
    want = plan.adjoint(g, g)
    assert torch.equal(plan.adjoint(torch.conj(torch.conj(g).resolve_conj()), g.to(torch.complex128)), want)
    assert torch.equal(plan.adjoint(g.transpose(-1, -2).contiguous().transpose(-1, -2), g), want)


# (dtype, padtype, l1_norm, N, fs, B, rpadded)
GRAD_CASES = [
    ('float32', 'reflect', True, 300, 1., 2, False),
    ('float64', 'zero', False, 300, 2., 0, False),
    ('float32', None, True, 301, 1., 1, False),
    ('float64', 'symmetric', True, 300, 1., 2, True),
]


@pytest.mark.parametrize('case', GRAD_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_cwt_gradient_through_dWx(S, case):
    """`x.grad` of a loss over `Wx` and `dWx` of `cwt(x, derivative=True)` against torch.autograd
    through the float64 torch statement of the same map. (Before `dWx` carried a gradient its
    term was missing from `x.grad`.)"""
    import torch
    from ssqueezepy_amd import _cwt
    dtype, padtype, l1_norm, N, fs, B, rpadded = case
    tol = TOL[dtype]
    rng = np.random.default_rng(7)
    wav = _wavelet(S, dtype, l1_norm)
    x0 = torch.as_tensor(np.stack([two_chirps(N, 3 + b) for b in range(max(B, 1))]) if B else two_chirps(N, 3),
                         dtype=_tdt(dtype), device=DEV)
    kw = dict(nv=8, padtype=padtype, l1_norm=l1_norm, fs=fs, derivative=True, rpadded=rpadded)
    _cwt.clear_plan_cache()
    x = x0.clone().requires_grad_(True)
    Wx, scales, dWx = S.cwt(x, wav, **kw)
    assert Wx.requires_grad and dWx.requires_grad
    assert Wx.grad_fn is not None and dWx.grad_fn is not None
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    cols = plan.M if (rpadded and padtype is not None) else N
    assert tuple(Wx.shape) == ((B,) if B else ()) + (plan.na, cols) == tuple(dWx.shape)
    wgt = torch.as_tensor(rng.random((plan.na, cols)) + 0.5, dtype=torch.float64, device=DEV)
    wgt2 = torch.as_tensor(rng.random((plan.na, cols)) + 0.5, dtype=torch.float64, device=DEV)
    _loss(Wx, dWx, wgt.to(_tdt(dtype)), wgt2.to(_tdt(dtype))).backward()
    assert plan._psih_dev is None

    xr = x0.to(torch.float64).clone().requires_grad_(True)
    Wr, dWr = torch_cwt(plan, xr, rpadded and padtype is not None)
    assert relmax(_np(Wx), _np(Wr)) <= tol
    print("measured: cwt forward dWx", case, relmax(_np(dWx), _np(dWr)))
    _loss(Wr, dWr, wgt, wgt2).backward()
    err = relmax(_np(x.grad).astype(np.float64), _np(xr.grad))
    # the share of the gradient that comes through dWx: what is missing when dWx is detached
    xw = x0.to(torch.float64).clone().requires_grad_(True)
    Ww, dWw = torch_cwt(plan, xw, rpadded and padtype is not None)
    _loss(Ww, dWw.detach(), wgt, wgt2).backward()
    print("measured: cwt gradient through dWx", case, err, "dWx term", relmax(_np(xw.grad), _np(xr.grad)))
    assert err <= 20 * tol

    # a loss over dWx alone, and one over Wx alone (the other gradient is None, not zeros)
    for pick in (0, 1):
        xa = x0.clone().requires_grad_(True)
        Wa, _, dWa = S.cwt(xa, wav, **kw)
        xb = x0.to(torch.float64).clone().requires_grad_(True)
        Wb, dWb = torch_cwt(plan, xb, rpadded and padtype is not None)
        if pick:
            (torch.abs(dWa)**2 * wgt2.to(_tdt(dtype))).sum().backward()
            (torch.abs(dWb)**2 * wgt2).sum().backward()
        else:
            (torch.abs(Wa)**2 * wgt.to(_tdt(dtype))).sum().backward()
            (torch.abs(Wb)**2 * wgt).sum().backward()
        assert relmax(_np(xa.grad).astype(np.float64), _np(xb.grad)) <= 20 * tol
    _cwt.clear_plan_cache()


# (dtype, padtype, l1_norm, N, nv, B, block rows wanted)
INNER_CASES = [
    ('float32', 'reflect', True, 300, 8, 2, False),
    ('float64', 'zero', False, 301, 8, 1, False),
    ('float32', None, True, 301, 8, 2, False),
    ('float32', 'reflect', True, 5000, 4, 1, True),             # rows on the block path
]


@pytest.mark.parametrize('case', INNER_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_cwt_inner_product_identity(S, case):
    """Re <A x, g> = <x, A^H g> with A the plan's OWN forward (`Wx` and `dWx`; the block kernels
    where the plan has them), `rpadded` off and on: the adjoint of the exact bank agrees with the
    fast forward within the suite's tolerance. `g` = weights x the forward's output + noise, so
    that the product is not a sum that cancels."""
    import torch
    dtype, padtype, l1_norm, N, nv, B, blocks = case
    rng = np.random.default_rng(N)
    plan = _plan(S, dtype, N, padtype, l1_norm, max_batch=B, nv=nv)
    if blocks:
        assert plan.block_rows > 0, plan.algo
    x = torch.as_tensor(np.stack([two_chirps(N, 11 + b) for b in range(B)]), dtype=_tdt(dtype), device=DEV)
    for rpadded in ((False, True) if padtype is not None else (False,)):
        out = plan.execute(x, want_dWx=True, rpadded=rpadded)
        W, dW = out['Wx'], out['dWx']
        g = []
        for t in (W, dW):
            t64 = t.to(torch.complex128)
            noise = _random_c(rng, tuple(t.shape), 'float64') * float(torch.abs(t64).max())
            wg = torch.as_tensor(rng.random(tuple(t.shape)) + 0.5, dtype=torch.float64, device=DEV)
            g.append((wg * t64 + 0.1 * noise).to(_tdt(dtype, True)))
        gx = plan.adjoint(g[0], g[1], rpadded=rpadded)
        lhs = sum(float((t.to(torch.complex128) * torch.conj(v.to(torch.complex128))).real.sum())
                  for t, v in zip((W, dW), g))
        rhs = float((x.to(torch.float64) * gx.to(torch.float64)).sum())
        err = abs(lhs - rhs) / abs(lhs)
        print("measured: cwt inner product", case, rpadded, plan.algo, err)
        assert err <= 20 * TOL[dtype]


@pytest.mark.parametrize('dtype,padtype,N', [('float32', 'reflect', 300), ('float64', 'symmetric', 301),
                                             ('float32', None, 301)])
def test_cwt_adjoint_batch_and_repeat(S, dtype, padtype, N):
    """Slice b of a batched adjoint has the bits of the single call on signal b; two identical
    calls have the same bits; the same on a cached plan made for a larger batch."""
    import torch
    from ssqueezepy_amd import _cwt
    rng = np.random.default_rng(5)
    plan = _plan(S, dtype, N, padtype, max_batch=3)
    gW, gdW = [_random_c(rng, (3, plan.na, N), dtype) for _ in range(2)]
    for a, d in ((gW, gdW), (gW, None), (None, gdW)):
        out = plan.adjoint(a, d)
        assert torch.equal(out, plan.adjoint(a, d)), "the adjoint is not deterministic"
        for b in range(3):
            one = plan.adjoint(None if a is None else a[b], None if d is None else d[b])
            assert torch.equal(out[b], one), b
    # batch < max_batch on a cached plan: the plan `cwt` made for four signals takes two
    _cwt.clear_plan_cache()
    wav = _wavelet(S, dtype, True)
    x4 = torch.as_tensor(np.stack([two_chirps(N, b) for b in range(4)]), dtype=_tdt(dtype), device=DEV)
    S.cwt(x4, wav, nv=8, padtype=padtype)
    cached = next(iter(_cwt._PLAN_CACHE.values()))
    assert cached.max_batch == 4 and cached.na == plan.na
    x2 = x4[:2].clone().requires_grad_(True)
    W2, _, dW2 = S.cwt(x2, wav, nv=8, padtype=padtype, derivative=True)
    assert len(_cwt._PLAN_CACHE) == 1 and next(iter(_cwt._PLAN_CACHE.values())) is cached
    (torch.conj(gW[:2]) * W2 + torch.conj(gdW[:2]) * dW2).real.sum().backward()
    assert torch.equal(x2.grad, cached.adjoint(gW[:2], gdW[:2]))
    assert torch.equal(x2.grad, plan.adjoint(gW, gdW)[:2])
    _cwt.clear_plan_cache()


@pytest.mark.parametrize('which', ['cwt', 'ssq_cwt'])
def test_backward_builds_no_dense_bank(S, which):
    """After `loss.backward()` through `cwt` / `ssq_cwt` on a fresh plan no dense bank exists, and
    the plan's device memory has grown by no more than its product workspace budget (2 GiB; a
    plan of this size: its whole product workspace, the spectrum sums and the small tables)."""
    import torch
    from ssqueezepy_amd import _cwt
    N = 300
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    _cwt.clear_plan_cache()
    x = torch.as_tensor(np.stack([two_chirps(N, 1), two_chirps(N, 2)]), dtype=torch.float32,
                        device=DEV).requires_grad_(True)
    if which == 'cwt':
        Wx, _, dWx = S.cwt(x, wav, nv=8, derivative=True)
        loss = (torch.abs(Wx)**2).sum() + (torch.abs(dWx)**2).sum()
    else:
        Tx, Wx, *_ = S.ssq_cwt(x, wav, nv=8)
        loss = (torch.abs(Tx)**2).sum() + Wx.real.sum()
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    before = plan.device_bytes
    loss.backward()
    assert x.grad is not None and float(torch.abs(x.grad).max()) > 0
    assert plan._psih_dev is None, "the backward built a dense bank"
    grown = plan.device_bytes - before
    per_row = 2 * plan.M * 8
    workspace = max(1, min(plan.na, BUDGET // per_row)) * per_row
    print("measured: plan bytes grown by the backward", which, grown, "product workspace", workspace)
    assert 0 <= grown <= BUDGET
    _cwt.clear_plan_cache()


def test_cwt_adjoint_abi(S):
    """ABI 108: `ssq_cwt_adjoint` is exported and bound; both gradients NULL and a batch above
    max_batch return non-zero and leave a message in `ssq_last_error`."""
    import torch
    from ssqueezepy_amd import _lib, algos
    lib = _lib.load()
    assert lib.ssq_version() >= 108 and _lib.ABI_VERSION >= 108
    assert 'ssq_cwt_adjoint' in _lib.EXPORTS and hasattr(lib, 'ssq_cwt_adjoint')
    assert lib.ssq_cwt_adjoint.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    plan = _plan(S, 'float32', 300, 'reflect', max_batch=2)
    g = _random_c(np.random.default_rng(1), (3, plan.na, 300), 'float32')
    gx = torch.zeros((3, 300), dtype=torch.float32, device=DEV)
    for args in ((None, None, gx.data_ptr(), 1), (g.data_ptr(), None, gx.data_ptr(), 3),
                 (g.data_ptr(), g.data_ptr(), gx.data_ptr(), 0), (g.data_ptr(), None, None, 1)):
        rc = lib.ssq_cwt_adjoint(plan._h, *args, 0, algos.stream())
        assert rc != 0, args
        msg = lib.ssq_last_error()
        assert msg and len(msg.decode()) > 0
    assert float(torch.abs(gx).max()) == 0, "a refused call wrote its output"
    assert lib.ssq_cwt_adjoint(plan._h, g.data_ptr(), None, gx.data_ptr(), 2, 0, algos.stream()) == 0
    assert torch.equal(gx[:2], plan.adjoint(g[:2]))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_ssq_cwt_end_to_end(S, dtype):
    """`x.grad` of sum |Tx|^2 + sum Re Wx through `ssq_cwt` on a batch of two: the gather of
    2 Tx through the bins `ssqueeze_fast(get_k=True)` reports (as test_ssq_cwt_gradient builds
    it), then the closed form; `dWx` of `get_dWx=True` stays outside the graph."""
    import torch
    from ssqueezepy_amd import _cwt
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    A = S.algos
    N, B = 400, 2
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    x0 = np.stack([two_chirps(N, 5 + b) for b in range(B)])
    x0[:, N // 3: N // 3 + N // 4] = 0          # a stretch without signal: points below gamma
    x0 = torch.as_tensor(x0, dtype=_tdt(dtype), device=DEV)
    kw = dict(scales='log', nv=8, gamma=1e-2)
    _cwt.clear_plan_cache()
    x = x0.clone().requires_grad_(True)
    Tx, Wx, ssq_freqs, scl, dWx = S.ssq_cwt(x, wav, get_dWx=True, **kw)
    assert Tx.requires_grad and Wx.requires_grad and not dWx.requires_grad
    (Tx.abs().pow(2).sum() + Wx.real.sum()).backward()
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    assert plan._psih_dev is None

    _, sf, const, grid, _ = _ssq_design(wav, 'log', 8, N, 1., None, 'peak', True)
    _, k = A.ssqueeze_fast(Wx.detach(), dWx, sf, const, grid != 2, True, kw['gamma'], get_k=True)
    k = k.to(torch.int64)
    assert 0.05 <= float((k < 0).double().mean()) <= 0.95
    cv = torch.as_tensor(np.broadcast_to(np.asarray(const, dtype=np.float64), (Wx.shape[-2],)).copy(),
                         device=DEV)[:, None]
    picked = torch.gather(2 * Tx.detach().to(torch.complex128), -2, k.clamp(min=0))
    gW = 1. + torch.where(k >= 0, picked * cv, torch.zeros((), dtype=torch.complex128, device=DEV))
    want = np.stack([closed_form(plan, _np(gW[b]), None, False, x0.device) for b in range(B)])
    err = relmax(_np(x.grad).astype(np.float64), want)
    print("measured: ssq_cwt end to end", dtype, err)
    assert err <= 20 * TOL[dtype]
    _cwt.clear_plan_cache()


def test_full_size_cwt_adjoint(S):
    """The benchmark's shape (N = 160 000, its 300 scales, float32) on a batch of two: the gradient
    of a loss over `Wx` and `dWx` against the float64 torch statement, one signal at a time."""
    import torch
    from ssqueezepy_amd import _cwt
    N, na, B = 160000, 300, 2
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    scales = S.process_scales('log', N, wav, nv=32)[:na]
    rng = np.random.default_rng(2)
    x0 = torch.as_tensor(np.stack([two_chirps(N, 20 + b) for b in range(B)]), dtype=torch.float32, device=DEV)
    wgt = torch.as_tensor(rng.random((1, N)) + 0.5, dtype=torch.float64, device=DEV)
    wgt2 = torch.as_tensor(rng.random((1, N)) + 0.5, dtype=torch.float64, device=DEV)
    _cwt.clear_plan_cache()
    x = x0.clone().requires_grad_(True)
    Wx, _, dWx = S.cwt(x, wav, scales=scales, derivative=True)
    assert tuple(Wx.shape) == (B, na, N) and dWx.requires_grad
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    before = plan.device_bytes
    _loss(Wx, dWx, wgt.float(), wgt2.float()).backward()
    assert plan._psih_dev is None
    grown = plan.device_bytes - before
    assert grown <= BUDGET, grown           # (the product workspace, rocFFT's work area of one pass, the spectrum sums)
    del Wx, dWx
    worst = 0.
    for b in range(B):
        xr = x0[b].to(torch.float64).clone().requires_grad_(True)
        Wr, dWr = torch_cwt(plan, xr)
        _loss(Wr, dWr, wgt, wgt2).backward()
        worst = max(worst, relmax(_np(x.grad[b]).astype(np.float64), _np(xr.grad)))
        del Wr, dWr
    print("measured: full-size cwt gradient (N=160000, 300 scales, float32, B=2)", worst,
          "plan bytes grown by the backward", grown)
    assert worst <= 20 * TOL['float32']
    _cwt.clear_plan_cache()
