# -*- coding: utf-8 -*-
"""Gradients of `stft`, `ssq_stft` and `ssq_cwt` (torch.autograd through the adjoint HIP kernels
`ssq_stft_adjoint` and `ssq_ssqueeze_adjoint`).

The STFT is linear in `x`: its backward is checked against torch.autograd through a plain torch
statement of the same map (pad gather, `unfold`, window, `torch.fft.rfft`), evaluated in float64 so
that the reference's own rounding stays out of the comparison, and against the closed form of the
adjoint. `Tx` is piecewise linear in `Wx` (the bins are integers): its backward is the gather
through the bins `ssqueeze_fast(get_k=True)` reports, checked exactly, then end to end.

Tolerances: the suite's 1e-5 (float32) / 1e-12 (float64) of the largest magnitude for a transform,
20 x that for an adjoint on top of a forward (the margin of test_cwt_is_differentiable).
"""
import os
import numpy as np
import pytest
from conftest import two_chirps

pytestmark = pytest.mark.gpu
TOL = {'float32': 1e-5, 'float64': 1e-12}
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _signal(N, B, seed=0, silent=False):
    x = np.stack([two_chirps(N, seed + b) for b in range(max(B, 1))])
    if silent:                       # a stretch without signal: points below gamma
        x[:, N // 3: N // 3 + N // 4] = 0
    return x if B else x[0]


from stft_lengths import pad_sources as _pad_sources      # noqa: E402  (source sample of every padded position)


def _windows(S, n_fft, win_len, modulated, fs, dtype):
    win, dwin = S.get_window(None, win_len or n_fft, n_fft, derivative=True, dtype=dtype)
    if modulated:
        win, dwin = np.fft.ifftshift(win), np.fft.ifftshift(dwin) * fs
    return win.astype(dtype), dwin.astype(dtype)       # (the plan's: rounded to the data dtype)


def torch_stft(S, x, n_fft, hop, win_len, padtype, modulated, fs, dtype):
    """The STFT as torch ops on a float64 copy of `x` (differentiable): Sx, dSx."""
    import torch
    N = x.shape[-1]
    win, dwin = [torch.as_tensor(w.astype(np.float64), device=x.device)
                 for w in _windows(S, n_fft, win_len, modulated, fs, dtype)]
    src = torch.as_tensor(_pad_sources(S, N, n_fft, padtype), device=x.device)
    xp = torch.where(src >= 0, x[..., src.clamp(min=0)], torch.zeros((), dtype=x.dtype, device=x.device))
    fr = xp.unfold(-1, n_fft, hop)
    if modulated:
        fr = torch.fft.ifftshift(fr, dim=-1)
    return (torch.fft.rfft(fr * win, dim=-1).transpose(-1, -2),
            torch.fft.rfft(fr * dwin, dim=-1).transpose(-1, -2))


def _stft_loss(Sx, dSx, wgt, wgt2):
    import torch
    loss = (torch.abs(Sx)**2 * wgt).sum() + (Sx.real * wgt).sum()
    if dSx is not None:
        loss = loss + (torch.abs(dSx)**2 * wgt2).sum() + (dSx.imag * wgt2).sum()
    return loss


def _last_plan():
    from ssqueezepy_amd import _stft
    return list(_stft._PLAN_CACHE.values())[-1]


# (dtype, n_fft, hop, padtype, modulated, win_len, N, B [0: 1-D], derivative, fs, algo)
STFT_CASES = [
    ('float32', 128, 1, 'reflect', True, None, 500, 2, True, 1., 'fused'),
    ('float32', 128, 3, 'zero', False, None, 500, 0, False, 1., 'fused'),
    ('float32', 128, 32, 'symmetric', True, 100, 501, 2, True, 2., 'fused'),
    ('float32', 128, 3, 'wrap', True, None, 77, 1, True, 1., 'fused'),
    ('float32', 128, 1, 'replicate', False, 90, 300, 0, True, 1., 'fused'),
    ('float32', 1024, 1, 'wrap', True, None, 300, 0, False, 1., 'fused'),
    ('float32', 1024, 3, 'replicate', False, None, 700, 2, True, 1., 'fused'),
    ('float32', 1024, 256, 'reflect', True, 800, 3001, 2, True, 1., 'fused'),
    ('float32', 1024, 256, 'symmetric', False, None, 700, 0, False, 1., 'fused'),
    ('float32', 1024, 1, 'reflect', True, None, 1500, 1, True, 1., 'fused'),
    ('float32', 1024, 3, 'zero', True, 1000, 1001, 0, False, 1., 'fused'),
    ('float32', 598, 7, 'reflect', True, None, 1000, 2, True, 1., 'fused-mixed-radix'),
    ('float32', 101, 5, 'symmetric', True, None, 333, 0, True, 1., None),
    ('float64', 256, 5, 'reflect', True, None, 700, 2, True, 1., 'rocfft'),
    ('float64', 100, 3, 'wrap', False, 64, 301, 0, True, 1., 'rocfft'),
    ('float64', 101, 4, 'symmetric', True, None, 150, 2, False, 3., 'rocfft'),
    ('float64', 128, 1, 'replicate', True, None, 200, 0, True, 1., 'rocfft'),
    ('float64', 64, 16, 'zero', True, None, 250, 1, True, 1., 'rocfft'),
]


@pytest.mark.parametrize('case', STFT_CASES, ids=lambda c: '-'.join(str(v) for v in c[:8]))
def test_stft_gradient_vs_torch(S, case):
    """`x.grad` through `S.stft` against torch.autograd through the torch statement of the same
    map (float64), for the fused kernel (float32, n_fft a power of two) and the composed route;
    the forward first, at the suite's tolerance; two backward passes give the same bits."""
    import torch
    dtype, n_fft, hop, padtype, modulated, win_len, N, B, deriv, fs, algo = case
    tol = TOL[dtype]
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    rng = np.random.default_rng(n_fft + hop)
    x0 = torch.as_tensor(_signal(N, B, seed=hop), dtype=tdt, device=DEV)
    kw = dict(n_fft=n_fft, win_len=win_len, hop_len=hop, padtype=padtype, modulated=modulated,
              fs=fs, dtype=dtype)
    n_hops = (N - 1) // hop + 1
    wgt = torch.as_tensor(rng.random((n_fft // 2 + 1, n_hops)) + 0.5, dtype=torch.float64, device=DEV)
    wgt2 = torch.as_tensor(rng.random((n_fft // 2 + 1, n_hops)) + 0.5, dtype=torch.float64, device=DEV)

    grads = []
    for rep in range(2):
        x = x0.clone().requires_grad_(True)
        res = S.stft(x, derivative=deriv, **kw)
        Sx, dSx = res if deriv else (res, None)
        assert Sx.requires_grad and Sx.grad_fn is not None
        assert dSx is None or dSx.requires_grad
        assert tuple(Sx.shape) == ((B,) if B else ()) + (n_fft // 2 + 1, n_hops)
        _stft_loss(Sx, dSx, wgt.to(tdt), wgt2.to(tdt)).backward()
        grads.append(x.grad.clone())
    if algo is not None:
        assert _last_plan().algo == algo
    assert torch.equal(grads[0], grads[1]), "the backward is not deterministic"

    xr = x0.to(torch.float64).requires_grad_(True)
    Sr, dSr = torch_stft(S, xr, n_fft, hop, win_len, padtype, modulated, fs, dtype)
    assert relmax(_np(Sx), _np(Sr)) <= tol
    if deriv:
        assert relmax(_np(dSx), _np(dSr)) <= tol
    _stft_loss(Sr, dSr if deriv else None, wgt, wgt2).backward()
    err = relmax(_np(grads[0]).astype(np.float64), _np(xr.grad))
    print("measured: stft gradient", case[:8], err)
    assert err <= 20 * tol

    # the forward's bits do not depend on whether a gradient is asked for
    with torch.no_grad():
        res0 = S.stft(x0, derivative=deriv, **kw)
    S0 = res0[0] if deriv else res0
    assert not S0.requires_grad and torch.equal(S0, Sx.detach())


def _adjoint_closed_form(g, win, n_fft, hop, N, src, modulated):
    """pad^T (sum_t win * Re F^-1(g[:, t])), F^-1 the one-sided sum of the issue, in float64."""
    rows, n_hops = g.shape
    E = np.exp(2j * np.pi * np.outer(np.arange(n_fft), np.arange(rows)) / n_fft)
    fr = (E @ g.astype(np.complex128)).real * win.astype(np.float64)[:, None]     # (n_fft, n_hops)
    if modulated:
        fr = np.fft.fftshift(fr, axes=0)           # back from the transform's order to the frame's
    y = np.zeros(N + n_fft - 1)
    for t in range(n_hops):
        y[t * hop: t * hop + n_fft] += fr[:, t]
    gx = np.zeros(N)
    np.add.at(gx, src[src >= 0], y[src >= 0])
    return gx


@pytest.mark.parametrize('dtype,n_fft,hop,padtype,modulated,N', [
    ('float32', 128, 1, 'reflect', True, 300),
    ('float32', 256, 64, 'wrap', False, 1000),
    ('float32', 1024, 3, 'symmetric', True, 600),
    ('float32', 2048, 512, 'replicate', True, 3000),
    ('float32', 512, 7, 'zero', True, 999),
    ('float32', 598, 7, 'reflect', True, 700),
    ('float64', 100, 3, 'reflect', True, 301),
    ('float64', 101, 3, 'symmetric', True, 301),
])
def test_stft_adjoint_abi_vs_closed_form(S, dtype, n_fft, hop, padtype, modulated, N):
    """`ssq_stft_adjoint` (through `StftPlan.adjoint`) with gSx only, gdSx only and both, batched,
    against the closed form; the random gradients carry imaginary parts at DC and Nyquist, which
    must not contribute. An adjoint alone: the suite's tolerance for a transform."""
    import torch
    from ssqueezepy_amd import _lib, _stft
    assert hasattr(_lib.load(), 'ssq_stft_adjoint')
    rng = np.random.default_rng(n_fft)
    win, dwin = _windows(S, n_fft, None, modulated, 1., dtype)
    w0, dw0 = S.get_window(None, n_fft, n_fft, derivative=True, dtype=dtype)
    plan = _stft.StftPlan(N, n_fft, hop, w0, dw0, 1., padtype, modulated, dtype, max_batch=2)
    if dtype == 'float32' and n_fft & (n_fft - 1) == 0:
        assert plan.algo == 'fused'
    rows, n_hops = plan.rows, plan.n_hops
    cdt = torch.complex64 if dtype == 'float32' else torch.complex128
    g = [(rng.standard_normal((2, rows, n_hops)) + 1j * rng.standard_normal((2, rows, n_hops)))
         for _ in range(2)]
    gS, gD = [torch.as_tensor(v, dtype=cdt, device=DEV) for v in g]
    src = _pad_sources(S, N, n_fft, padtype)
    ref = [[_adjoint_closed_form(_np(t[b]), w, n_fft, hop, N, src, modulated) for b in range(2)]
           for t, w in ((gS, win), (gD, dwin))]
    for a, d, want in ((gS, None, np.stack(ref[0])), (None, gD, np.stack(ref[1])),
                       (gS, gD, np.stack(ref[0]) + np.stack(ref[1]))):
        out = plan.adjoint(a, d)
        assert tuple(out.shape) == (2, N)
        err = relmax(_np(out).astype(np.float64), want)
        print("measured: stft adjoint", dtype, n_fft, hop, padtype, a is not None, d is not None, err)
        assert err <= TOL[dtype]
        assert torch.equal(out, plan.adjoint(a, d))
    one = plan.adjoint(gS[1], None)                      # a single signal
    assert tuple(one.shape) == (N,) and relmax(_np(one).astype(np.float64), ref[0][1]) <= TOL[dtype]


def _freq_grid(kind, na, lo, hi):
    if kind == 'log':
        return np.logspace(np.log10(lo), np.log10(hi), na)
    if kind == 'log-piecewise':
        sf = np.logspace(np.log10(lo), np.log10(hi), 2 * na)
        return np.hstack([sf[:na // 2], sf[na // 2 + 3 - 1::3]])
    return np.linspace(0, hi, na)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('form', ['cwt', 'stft'])
def test_ssqueeze_adjoint_is_the_gather(S, dtype, form):
    """`ssq_ssqueeze_adjoint(gTx=G)` == `cst[a] * G[k[a, b], b]` (0 where k == -1), exactly, with
    the `k` `ssqueeze_fast(get_k=True)` reports for the forward's own `Wx`, `dWx`; a float64
    weight vector on float32 data: the double product rounded once."""
    import torch
    A = S.algos
    from ssqueezepy_amd import _lib
    assert hasattr(_lib.load(), 'ssq_ssqueeze_adjoint')
    rng = np.random.default_rng(5)
    N, B = 400, 2
    x = _signal(N, B, seed=3, silent=True).astype(dtype)
    if form == 'cwt':
        Wx, _, dWx = S.cwt(x, S.Wavelet(('gmw', {'dtype': dtype})), nv=8, derivative=True)
        Sfs, grids, lo = None, ('log', 'log-piecewise', 'linear'), 2e-3
    else:
        Wx, dWx = S.stft(x, n_fft=128, hop_len=2, derivative=True, dtype=dtype)
        Sfs, grids, lo = np.linspace(0, .5, Wx.shape[-2]).astype(dtype), ('linear', 'log'), 2e-3
    na, n = Wx.shape[-2:]
    gamma = 2e-2 * float(torch.abs(Wx).max())
    cdt = Wx.dtype
    G = torch.as_tensor(rng.standard_normal((B, na, n)) + 1j * rng.standard_normal((B, na, n)),
                        dtype=cdt, device=DEV)
    prior = torch.as_tensor(rng.standard_normal((B, na, n)) + 0j, dtype=cdt, device=DEV)
    fractions = []
    for grid in grids:
        sf = _freq_grid(grid, na, lo, .5)
        consts = [('scalar', np.log(2) / 8), ('vec', (np.log(2) / np.linspace(8, 32, na)).astype(dtype))]
        if dtype == 'float32':
            consts.append(('vec64', np.log(2) / np.linspace(8, 32, na)))
        for flipud in (False, True):
            for cname, const in consts:
                args = (sf, const, grid != 'linear', flipud, gamma)
                _, k = A.ssqueeze_fast(Wx, dWx, *args, Sfs=Sfs, get_k=True)
                k = _np(k).astype(np.int64)
                fractions.append(float((k < 0).mean()))
                Gn = _np(G)
                picked = np.take_along_axis(Gn, np.maximum(k, 0), axis=-2)
                cv = np.broadcast_to(np.asarray(const), (na,))
                if cname == 'vec64':
                    want = (picked.astype(np.complex128) * cv[:, None]).astype(Gn.dtype)
                else:
                    cv = cv.astype(dtype)[:, None]
                    want = (picked.real * cv + 1j * (picked.imag * cv)).astype(Gn.dtype)
                want = np.where(k >= 0, want, 0)
                got = A.ssqueeze_adjoint(Wx, dWx, G, *args, Sfs=Sfs)
                assert np.array_equal(_np(got), want), (grid, flipud, cname)
                acc = prior.clone()
                A.ssqueeze_adjoint(Wx, dWx, G, *args, Sfs=Sfs, out=acc, accumulate=True)
                assert np.array_equal(_np(acc), _np(prior) + want), (grid, flipud, cname, 'accumulate')
                # a single signal of the batch
                got1 = A.ssqueeze_adjoint(Wx[1], dWx[1], G[1], *args, Sfs=Sfs)
                assert np.array_equal(_np(got1), want[1])
    print("measured: share of points below gamma", form, dtype, min(fractions), max(fractions))
    assert any(0.05 <= f <= 0.95 for f in fractions), fractions


def _ssq_loss(Tx, Wx, G, wgt):
    import torch
    return (torch.conj(G) * Tx).real.sum() + (torch.abs(Wx)**2 * wgt).sum()


@pytest.mark.parametrize('dtype,n_fft,hop,B', [('float32', 128, 2, 2), ('float32', 256, 64, 0),
                                               ('float64', 100, 3, 2)])
def test_ssq_stft_gradient(S, dtype, n_fft, hop, B):
    """`x.grad` through `ssq_stft` for the loss Re sum conj(G) Tx + sum |Sx|^2 wgt: the torch
    statement's adjoint applied to 2 wgt Sx + cst G[k], `k` from `ssqueeze_fast(get_k=True)`."""
    import torch
    A = S.algos
    tol = TOL[dtype]
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    N = 600
    rng = np.random.default_rng(11)
    x0 = torch.as_tensor(_signal(N, B, seed=7, silent=True), dtype=tdt, device=DEV)
    kw = dict(n_fft=n_fft, hop_len=hop, dtype=dtype, gamma=1e-3)
    grads = []
    for rep in range(2):
        x = x0.clone().requires_grad_(True)
        Tx, Sx, ssq_freqs, Sfs, dSx = S.ssq_stft(x, get_dWx=True, **kw)
        assert Tx.requires_grad and Sx.requires_grad and not dSx.requires_grad
        if rep == 0:
            G = torch.as_tensor(rng.standard_normal(Tx.shape) + 1j * rng.standard_normal(Tx.shape),
                                dtype=Tx.dtype, device=DEV)
            wgt = torch.as_tensor(rng.random(Tx.shape) + 0.5, dtype=tdt, device=DEV)
        _ssq_loss(Tx, Sx, G, wgt).backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1]), "the backward is not deterministic"
    with torch.no_grad():
        T0, S0, *_ = S.ssq_stft(x0, **kw)
    assert not T0.requires_grad and torch.equal(S0, Sx.detach())
    assert relmax(_np(Tx), _np(T0)) <= 1e-6

    const = ssq_freqs[1] - ssq_freqs[0]
    _, k = A.ssqueeze_fast(Sx.detach(), dSx, ssq_freqs, const, False, False, kw['gamma'], Sfs=Sfs,
                           get_k=True)
    k = k.to(torch.int64)
    assert 0.05 <= float((k < 0).double().mean()) <= 0.95
    gS = 2 * wgt * Sx.detach() + torch.where(k >= 0, float(const) * torch.gather(G, -2, k.clamp(min=0)),
                                             torch.zeros((), dtype=G.dtype, device=DEV))
    xr = x0.to(torch.float64).requires_grad_(True)
    Sr, _ = torch_stft(S, xr, n_fft, hop, None, 'reflect', True, 1., dtype)
    (torch.conj(gS.to(torch.complex128)) * Sr).real.sum().backward()
    err = relmax(_np(grads[0]).astype(np.float64), _np(xr.grad))
    print("measured: ssq_stft gradient", dtype, n_fft, hop, err)
    assert err <= 20 * tol


@pytest.mark.parametrize('dtype,scales,B', [('float32', 'log', 2), ('float32', 'log-piecewise', 0),
                                            ('float64', 'log', 0), ('float32', 'linear', 0)])
def test_ssq_cwt_gradient(S, dtype, scales, B):
    """`x.grad` through `ssq_cwt` for the loss Re sum conj(G) Tx + sum |Wx|^2 wgt: the tested
    `CwtPlan.adjoint` applied to 2 wgt Wx + cst G[k], `k` from `ssqueeze_fast(get_k=True)`."""
    import torch
    from ssqueezepy_amd import _cwt
    A = S.algos
    tol = TOL[dtype]
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    N = 400
    rng = np.random.default_rng(13)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    x0 = torch.as_tensor(_signal(N, B, seed=5, silent=True), dtype=tdt, device=DEV)
    kw = dict(scales=scales, nv=8, gamma=1e-2)
    _cwt.clear_plan_cache()
    grads = []
    for rep in range(2):
        x = x0.clone().requires_grad_(True)
        Tx, Wx, ssq_freqs, scl, dWx = S.ssq_cwt(x, wav, get_dWx=True, **kw)
        assert Tx.requires_grad and Wx.requires_grad and not dWx.requires_grad
        if rep == 0:
            G = torch.as_tensor(rng.standard_normal(Tx.shape) + 1j * rng.standard_normal(Tx.shape),
                                dtype=Tx.dtype, device=DEV)
            wgt = torch.as_tensor(rng.random(Tx.shape) + 0.5, dtype=tdt, device=DEV)
        _ssq_loss(Tx, Wx, G, wgt).backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1]), "the backward is not deterministic"
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    with torch.no_grad():
        T0, W0, *_ = S.ssq_cwt(x0, wav, **kw)
    assert not T0.requires_grad and torch.equal(W0, Wx.detach())
    assert relmax(_np(Tx), _np(T0)) <= 1e-6

    from ssqueezepy_amd._ssq_cwt import _ssq_design
    _, sf, const, grid, _ = _ssq_design(wav, scales, 8, N, 1., None, 'peak', True)
    _, k = A.ssqueeze_fast(Wx.detach(), dWx, sf, const, grid != 2, True, kw['gamma'], get_k=True)
    k = k.to(torch.int64)
    assert 0.05 <= float((k < 0).double().mean()) <= 0.95
    cv = torch.as_tensor(np.broadcast_to(np.asarray(const, dtype=np.float64), (Wx.shape[-2],)).copy(),
                         device=DEV)[:, None]
    picked = torch.gather(G, -2, k.clamp(min=0))
    gW = 2 * wgt * Wx.detach() + torch.where(k >= 0, (picked.to(torch.complex128) * cv).to(G.dtype),
                                             torch.zeros((), dtype=G.dtype, device=DEV))
    want = plan.adjoint(gW)
    err = relmax(_np(grads[0]), _np(want))
    print("measured: ssq_cwt gradient", dtype, scales, err)
    assert err <= 20 * tol
    _cwt.clear_plan_cache()


FD_EPS = 1e-7
FD_CWT_ERR = 6.4e-9     # measured for `cwt` alone (see the docstring below)


@pytest.mark.parametrize('which', ['ssq_cwt', 'ssq_stft'])
def test_ssq_gradient_vs_finite_difference(S, which):
    """float64: (L(x + eps v) - L(x - eps v)) / (2 eps) along a random direction v against
    <x.grad, v>, for L = Re sum conj(G) Tx + sum |Wx|^2 wgt. Valid only while no bin flips: the
    three bin maps (at x, x + eps v, x - eps v) are asserted equal first (seed and eps chosen so).

    The bound is 10 x the error of the same check on `cwt` alone (the loss sum |Wx|^2 wgt, whose
    adjoint is already trusted) at the same eps = 1e-7; both losses are quadratic, so the central
    difference has no truncation error and what is left is the rounding of the two loss values,
    which scales with the loss. Measured relative errors |fd - <grad, v>| / |<grad, v>|:
    cwt alone 8.6e-10 .. 6.4e-9 over six directions v (seeds 0..5; at eps = 1e-6 they are ten times
    smaller, as rounding predicts) on the host build of the kernels -- the bound is 10 x the
    largest, 6.4e-8; there ssq_cwt 1.4e-8, ssq_stft 4.5e-9. On the MI355X, with this test's v:
    cwt alone 7.5e-9, ssq_cwt 3.6e-9, ssq_stft 4.5e-9 (every run prints its own figures)."""
    import torch
    A = S.algos
    N = 300
    rng = np.random.default_rng(2)
    x0 = torch.as_tensor(_signal(N, 0, seed=9, silent=True), dtype=torch.float64, device=DEV)
    v = torch.as_tensor(rng.standard_normal(N), dtype=torch.float64, device=DEV)
    wav = S.Wavelet(('gmw', {'dtype': 'float64'}))
    gamma = 1e-2

    def run(x):
        if which == 'ssq_cwt':
            Tx, Wx, sf, _, dWx = S.ssq_cwt(x, wav, scales='log', nv=8, gamma=gamma, get_dWx=True)
            from ssqueezepy_amd._ssq_cwt import _ssq_design
            _, sfu, const, _, _ = _ssq_design(wav, 'log', 8, N, 1., None, 'peak', True)
            _, k = A.ssqueeze_fast(Wx.detach(), dWx, sfu, const, True, True, gamma, get_k=True)
        else:
            Tx, Wx, sf, Sfs, dWx = S.ssq_stft(x, n_fft=64, hop_len=2, gamma=gamma, dtype='float64',
                                              get_dWx=True)
            _, k = A.ssqueeze_fast(Wx.detach(), dWx, sf, sf[1] - sf[0], False, False, gamma, Sfs=Sfs,
                                   get_k=True)
        return Tx, Wx, k

    x = x0.clone().requires_grad_(True)
    Tx, Wx, k0 = run(x)
    G = torch.as_tensor(rng.standard_normal(Tx.shape) + 1j * rng.standard_normal(Tx.shape),
                        dtype=Tx.dtype, device=DEV)
    wgt = torch.as_tensor(rng.random(Tx.shape) + 0.5, dtype=torch.float64, device=DEV)
    _ssq_loss(Tx, Wx, G, wgt).backward()
    with torch.no_grad():
        Tp, Wp, kp = run(x0 + FD_EPS * v)
        Tm, Wm, km = run(x0 - FD_EPS * v)
        assert torch.equal(k0, kp) and torch.equal(k0, km), "a bin flipped: the check is void"
        fd = float(_ssq_loss(Tp, Wp, G, wgt) - _ssq_loss(Tm, Wm, G, wgt)) / (2 * FD_EPS)
    an = float((x.grad * v).sum())
    err = abs(fd - an) / abs(an)

    # the same check on cwt alone
    xc = x0.clone().requires_grad_(True)
    Wc, _ = S.cwt(xc, wav, scales='log', nv=8)
    wc = torch.as_tensor(np.random.default_rng(2).random(Wc.shape) + 0.5, dtype=torch.float64, device=DEV)
    (torch.abs(Wc)**2 * wc).sum().backward()
    with torch.no_grad():
        lp = (torch.abs(S.cwt(x0 + FD_EPS * v, wav, scales='log', nv=8)[0])**2 * wc).sum()
        lm = (torch.abs(S.cwt(x0 - FD_EPS * v, wav, scales='log', nv=8)[0])**2 * wc).sum()
    anc = float((xc.grad * v).sum())
    errc = abs(float(lp - lm) / (2 * FD_EPS) - anc) / abs(anc)
    print("measured: finite difference", which, "err", err, "cwt alone", errc)
    assert err <= 10 * FD_CWT_ERR


def test_no_gradient_when_none_is_asked_for(S):
    """No `grad_fn` under `torch.no_grad()`, for NumPy input, and -- silently, as before -- for the
    options whose gradient is not implemented; `Sx` / `Wx` do not depend on the request."""
    import torch
    N = 300
    xn = _signal(N, 0, seed=1).astype('float32')
    x = torch.as_tensor(xn, device=DEV).requires_grad_(True)
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    with torch.no_grad():
        assert not S.stft(x, n_fft=128).requires_grad
        assert not any(t.requires_grad for t in S.ssq_stft(x, n_fft=128)[:2])
        assert not any(t.requires_grad for t in S.ssq_cwt(x, wav, nv=8)[:2])
    for t in (S.stft(xn, n_fft=128), *S.ssq_stft(xn, n_fft=128)[:2], *S.ssq_cwt(xn, wav, nv=8)[:2]):
        assert isinstance(t, torch.Tensor) and not t.requires_grad and t.grad_fn is None
    # with a gradient: the documented outputs carry it, the others do not
    Sx, dSx = S.stft(x, n_fft=128, derivative=True)
    assert Sx.grad_fn is not None and dSx.grad_fn is not None
    Tx, Sx2, sf, Sfs = S.ssq_stft(x, n_fft=128)
    assert Tx.grad_fn is not None and Sx2.grad_fn is not None and isinstance(sf, np.ndarray)
    assert torch.equal(Sx2.detach(), Sx.detach())
    Tx, Wx, sf, scl = S.ssq_cwt(x, wav, nv=8)
    assert Tx.grad_fn is not None and Wx.grad_fn is not None and isinstance(scl, np.ndarray)
    assert torch.equal(Wx.detach(), S.ssq_cwt(xn, wav, nv=8)[1])
    # out of scope: no gradient on Tx, and no exception
    for kw in (dict(squeezing='abs'), dict(squeezing='lebesgue'), dict(get_w=True)):
        assert S.ssq_stft(x, n_fft=128, **kw)[0].grad_fn is None, kw
        assert S.ssq_cwt(x, wav, nv=8, **kw)[0].grad_fn is None, kw
    assert S.ssq_cwt(x, wav, nv=8, order=1)[0].grad_fn is None
