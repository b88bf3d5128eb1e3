# -*- coding: utf-8 -*-
"""Batched, differentiable inverses: `istft` (fused LDS kernel / composed route), `issq_stft`,
`issq_cwt` (with and without curves) and `icwt(one_int=True)`, through `ssq_istft_batch`,
`ssq_istft_adjoint`, `ssq_colsum_adjoint`, `ssq_band_colsum_batch`, `ssq_band_colsum_adjoint`.

`istft` is checked against an independent float64 statement in torch (`torch.fft.irfft`,
`fftshift`, overlap-add, window norm, trim) on this engine's own forward transform, its gradient
against torch.autograd through that statement and against the closed form; the column-sum and band
adjoints are exact and compared bit for bit.

Tolerances: `TOL` = 1e-5 (float32) / 1e-12 (float64) of the largest magnitude for a transform,
20 x `TOL` for an adjoint on top of a forward. The division by the window norm `wn` amplifies
rounding where `wn` is small, so every `TOL` case asserts ``wn.min() >= 0.5`` on the float64
statement before it compares (the default window is narrow: it inverts at small hops only, larger
hops use ``window='hann'``); `'hann'` at hop n_fft/2 (`wn` down to 0.16) is compared at 1e-4 / 1e-10,
the bound tests/test_gpu_inverse.py::test_istft_odd_sizes_and_window_powers uses for small norms.
"""
import os
import numpy as np
import pytest
from conftest import two_chirps
from test_gpu_autograd import torch_stft, _signal, _np, relmax

pytestmark = pytest.mark.gpu
TOL = {'float32': 1e-5, 'float64': 1e-12}
TOL_SMALL_NORM = {'float32': 1e-4, 'float64': 1e-10}
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
FUSED_SIZES = (128, 256, 512, 1024, 2048)


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == 'float64' else torch.float32


def _cdt(dtype):
    import torch
    return torch.complex128 if dtype == 'float64' else torch.complex64


def _win_powers(S, window, win_len, n_fft, win_exp, dtype):
    """window^a and window^(a+1) as `istft` forms them (in the data dtype)."""
    w = S.get_window(window, win_len or n_fft, n_fft=n_fft, dtype=dtype)
    wa = np.ones(n_fft, dtype=dtype) if win_exp == 0 else (w if win_exp == 1 else w ** win_exp)
    return wa, w ** (win_exp + 1)


def _window_norm(wa1, n_fft, hop, N):
    wn = np.zeros(N + n_fft - 1)
    for i in range((N - 1) // hop + 1):
        wn[i * hop:i * hop + n_fft] += wa1.astype(np.float64)
    return wn


def torch_istft(S, Sx, window, n_fft, win_len, hop, N, modulated, win_exp, dtype):
    """The inverse STFT as torch ops on a complex128 `Sx` (differentiable): x (..., N) float64, and
    the window norm of its N samples."""
    import torch
    wa, wa1 = _win_powers(S, window, win_len, n_fft, win_exp, dtype)
    n_hops = Sx.shape[-1]
    fr = torch.fft.irfft(Sx.transpose(-1, -2), n=n_fft, dim=-1)            # (..., n_hops, n_fft)
    if modulated:
        fr = torch.fft.fftshift(fr, dim=-1)
    fr = fr * torch.as_tensor(wa.astype(np.float64), device=Sx.device)
    total = N + n_fft - 1
    buflen = max(total, (n_hops - 1) * hop + n_fft)
    idx = (torch.arange(n_hops, device=Sx.device)[:, None] * hop
           + torch.arange(n_fft, device=Sx.device)[None, :]).reshape(-1)
    y = torch.zeros(Sx.shape[:-2] + (buflen,), dtype=torch.float64, device=Sx.device)
    y = y.index_add(-1, idx, fr.reshape(fr.shape[:-2] + (-1,)))[..., :total]
    wn = _window_norm(wa1, n_fft, hop, N)
    tiny = np.finfo(dtype).tiny
    wnt = torch.as_tensor(np.where(wn > tiny, wn, 1.), device=Sx.device)
    x = y / wnt
    half = n_fft // 2
    return x[..., half:half + N], wn[half:half + N]


def _x(N, B, dtype, seed=0):
    import torch
    return torch.as_tensor(_signal(N, B, seed=seed), dtype=_tdt(dtype), device=DEV)


# ------------------------------------------------------------------ 1. batch equals single
# (dtype, n_fft, hop, N): a fused and a composed shape per dtype (float64 is always composed)
BATCH_SHAPES = [('float32', 128, 16, 677), ('float32', 100, 7, 500),
                ('float64', 128, 16, 677), ('float64', 101, 5, 333)]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('dtype,n_fft,hop,N', BATCH_SHAPES)
def test_istft_batch_equals_single(S, dtype, n_fft, hop, N, B):
    """Slice b of `istft` on (B, rows, n_hops) has the bits of `istft` on slice b; the default
    `n_fft` and `N` come from the last two axes."""
    import torch
    x = _x(N, B, dtype, seed=3)
    Sx = S.stft(x, n_fft=n_fft, hop_len=hop, dtype=dtype, window='hann')
    assert Sx.shape[0] == B and Sx.ndim == 3
    kw = dict(window='hann', hop_len=hop)
    xb = S.istft(Sx, n_fft=n_fft, N=N, **kw)
    assert tuple(xb.shape) == (B, N)
    algo = S.algos.istft_algo(dtype, n_fft, Sx.shape[-1], hop, N)
    assert algo == ('fused' if (dtype, n_fft) == ('float32', 128) else 'rocfft')
    for b in range(B):
        assert torch.equal(xb[b], S.istft(Sx[b], n_fft=n_fft, N=N, **kw)), (b, algo)
    if n_fft % 2 == 0:
        xd = S.istft(Sx, **kw)                     # defaults: n_fft from shape[-2], N = hop * shape[-1]
        assert tuple(xd.shape) == (B, hop * Sx.shape[-1])
        assert torch.equal(xd[B - 1], S.istft(Sx[B - 1], **kw))
    err = relmax(_np(xb).astype(np.float64), _np(x).astype(np.float64))
    print("measured: istft round trip", dtype, n_fft, hop, N, B, algo, err)


def _curves(N, K, na, rng, B=None):
    shape = (N, K) if B is None else (B, N, K)
    cc = rng.integers(0, na, shape)
    cw = rng.integers(0, max(2, na // 6), shape)
    cc[..., N // 5, 0] = -1                         # "no curve here"
    return cc, cw


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_issq_batch_equals_single(S, dtype, B):
    """`issq_cwt` / `issq_stft` of a batch, without curves, with curves shared by the batch and
    with per-signal curves: every slice has the bits of the single call."""
    import torch
    N, na, K = 300, 33, 2
    rng = np.random.default_rng(B)
    Tx = torch.as_tensor(rng.standard_normal((B, na, N)) + 1j * rng.standard_normal((B, na, N)),
                         dtype=_cdt(dtype), device=DEV)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    inv = (lambda T, **kw: S.issq_cwt(T, wav, **kw)), (lambda T, **kw: S.issq_stft(T, n_fft=64, **kw))
    for f in inv:
        xb = f(Tx)
        assert tuple(xb.shape) == (B, N)
        for b in range(B):
            assert torch.equal(xb[b], f(Tx[b]))
        cc, cw = _curves(N, K, na, rng)
        xb = f(Tx, cc=cc, cw=cw)
        assert tuple(xb.shape) == (B, K + 1, N) and xb.dtype == torch.float64
        for b in range(B):
            assert torch.equal(xb[b], f(Tx[b], cc=cc, cw=cw))
        ccb, cwb = _curves(N, K, na, rng, B)
        xb = f(Tx, cc=ccb, cw=cwb)
        for b in range(B):
            assert torch.equal(xb[b], f(Tx[b], cc=ccb[b], cw=cwb[b]))
    # default n_fft of issq_stft from shape[-2]
    assert torch.equal(S.issq_stft(Tx), S.issq_stft(Tx, n_fft=64))
    with pytest.raises(ValueError):
        S.issq_cwt(Tx[0], wav, cc=ccb, cw=cwb)      # per-signal curves need a batch


# ------------------------------------------------------------------ 2. route
def test_istft_route(S):
    algo = S.algos.istft_algo
    for n_fft in FUSED_SIZES:
        for hop, N in ((1, 300), (n_fft // 4, 5 * n_fft + 37)):
            assert algo('float32', n_fft, (N - 1) // hop + 1, hop, N) == 'fused'
            assert algo('float64', n_fft, (N - 1) // hop + 1, hop, N) == 'rocfft'
            assert algo('float32', n_fft, (N - 1) // hop + 2, hop, N) == 'rocfft'    # frames do not match N
    for n_fft in (100, 101, 64, 598, 4096):
        assert algo('float32', n_fft, 300, 1, 300) == 'rocfft'


# ------------------------------------------------------------------ 3. fused istft vs the statement
# (window, hop as a function of n_fft, win_len as a function of n_fft)
WINDOW_CASES = {
    'default-hop1': (None, lambda n: 1, lambda n: None),
    'default-hop3': (None, lambda n: 3, lambda n: None),
    'hann-n/8': ('hann', lambda n: n // 8, lambda n: None),
    'hann-n/4': ('hann', lambda n: n // 4, lambda n: None),
    'hann0.78-n/8': ('hann', lambda n: n // 8, lambda n: int(round(0.78 * n))),
}


def _default_N(n_fft, hop):
    """5 n_fft + 37, one more where that is a multiple of the hop."""
    N = 5 * n_fft + 37
    return N + 1 if hop > 1 and N % hop == 0 else N


def _forward_and_statement(S, n_fft, window, win_len, hop, N, modulated, win_exp, B, dtype):
    x = _x(N, B, dtype, seed=hop % 7)
    kw = dict(window=window, n_fft=n_fft, win_len=win_len, hop_len=hop, modulated=modulated)
    import torch
    with torch.no_grad():
        Sx = S.stft(x, dtype=dtype, **kw)
    return Sx, kw


def check_istft_vs_statement(S, n_fft, wcase, N=None, dtype='float32', algo='fused', combos=None):
    import torch
    window, hopf, wlf = WINDOW_CASES[wcase]
    hop, win_len = hopf(n_fft), wlf(n_fft)
    N = N or _default_N(n_fft, hop)
    assert N % hop or hop == 1
    worst = 0.
    for modulated in (True, False):
        for win_exp in (0, 1, 2):
            for B in (0, 2):
                if combos is not None and (modulated, win_exp, B) not in combos:
                    continue
                Sx, kw = _forward_and_statement(S, n_fft, window, win_len, hop, N, modulated, win_exp, B, dtype)
                assert S.algos.istft_algo(dtype, n_fft, Sx.shape[-1], hop, N) == algo
                xr = S.istft(Sx, N=N, win_exp=win_exp, **kw)
                ref, wn = torch_istft(S, Sx.to(torch.complex128), window, n_fft, win_len, hop, N, modulated,
                                      win_exp, dtype)
                assert wn.min() >= 0.5, (wcase, n_fft, win_exp, wn.min())
                assert xr.shape == ref.shape and xr.dtype == _tdt(dtype)
                err = relmax(_np(xr).astype(np.float64), _np(ref))
                print("measured: istft vs statement", dtype, n_fft, wcase, N, modulated, win_exp, B,
                      "wn.min %.3g" % wn.min(), err)
                worst = max(worst, err)
                assert err <= TOL[dtype], (wcase, n_fft, modulated, win_exp, B, err)
    return worst


@pytest.mark.parametrize('wcase', list(WINDOW_CASES))
@pytest.mark.parametrize('n_fft', FUSED_SIZES)
def test_fused_istft_vs_statement(S, n_fft, wcase):
    """The fused kernel against the float64 statement: five sizes, `modulated` both ways,
    `win_exp` 0 / 1 / 2, single and batched, N = 5 n_fft + 37 (+ 1 where that is a multiple of the hop)."""
    check_istft_vs_statement(S, n_fft, wcase)


@pytest.mark.parametrize('n_fft', FUSED_SIZES)
def test_fused_istft_small_window_norm(S, n_fft, N=None):
    """`'hann'` at hop n_fft / 2: the window norm falls to ~0.16 at the ends; the bound of
    test_istft_odd_sizes_and_window_powers for small norms."""
    import torch
    hop, N = n_fft // 2, N or _default_N(n_fft, n_fft // 2)
    for win_exp in (0, 1):
        for B in (0, 2):
            Sx, kw = _forward_and_statement(S, n_fft, 'hann', None, hop, N, True, win_exp, B, 'float32')
            assert S.algos.istft_algo('float32', n_fft, Sx.shape[-1], hop, N) == 'fused'
            xr = S.istft(Sx, N=N, win_exp=win_exp, **kw)
            ref, wn = torch_istft(S, Sx.to(torch.complex128), 'hann', n_fft, None, hop, N, True, win_exp,
                                  'float32')
            err = relmax(_np(xr).astype(np.float64), _np(ref))
            print("measured: istft small norm", n_fft, win_exp, B, "wn.min %.3g" % wn.min(), err)
            assert err <= TOL_SMALL_NORM['float32']


# ------------------------------------------------------------------ 4. gradient of istft
def _x_loss(x, wgt):
    return (x ** 2 * wgt).sum() + (x * wgt).sum()


def check_istft_gradient(S, dtype, n_fft, window, win_len, hop, N, modulated, win_exp, B, algo):
    import torch
    tol = TOL[dtype]
    rng = np.random.default_rng(n_fft + hop)
    Sx0, kw = _forward_and_statement(S, n_fft, window, win_len, hop, N, modulated, win_exp, B, dtype)
    assert S.algos.istft_algo(dtype, n_fft, Sx0.shape[-1], hop, N) == algo
    wgt = torch.as_tensor(rng.random(N) + 0.5, dtype=torch.float64, device=DEV)
    grads = []
    for rep in range(2):
        Sx = Sx0.clone().requires_grad_(True)
        x = S.istft(Sx, N=N, win_exp=win_exp, **kw)
        assert x.requires_grad and x.grad_fn is not None
        _x_loss(x, wgt.to(_tdt(dtype))).backward()
        grads.append(Sx.grad.clone())
    assert torch.equal(torch.view_as_real(grads[0]), torch.view_as_real(grads[1])), "the backward is not deterministic"
    with torch.no_grad():
        x0 = S.istft(Sx0, N=N, win_exp=win_exp, **kw)
    assert x0.grad_fn is None and torch.equal(x0, x.detach())

    Sr = Sx0.to(torch.complex128).requires_grad_(True)
    xr, wn = torch_istft(S, Sr, window, n_fft, win_len, hop, N, modulated, win_exp, dtype)
    assert wn.min() >= 0.5, (n_fft, hop, win_exp, wn.min())
    assert relmax(_np(x).astype(np.float64), _np(xr)) <= tol
    _x_loss(xr, wgt).backward()
    g, gr = _np(grads[0]).astype(np.complex128), _np(Sr.grad)
    err = relmax(g, gr)
    print("measured: istft gradient", dtype, n_fft, window, win_len, hop, N, modulated, win_exp, B, algo, err)
    assert err <= 20 * tol
    if n_fft % 2 == 0:
        assert not g[..., 0, :].imag.any() and not g[..., n_fft // 2, :].imag.any()
    else:
        assert not g[..., 0, :].imag.any()


GRAD_COMBOS = [(True, 1, 2), (False, 0, 0), (True, 2, 0), (False, 1, 2), (True, 0, 2)]


@pytest.mark.parametrize('wcase', list(WINDOW_CASES))
@pytest.mark.parametrize('n_fft', FUSED_SIZES)
def test_fused_istft_gradient(S, n_fft, wcase):
    window, hopf, wlf = WINDOW_CASES[wcase]
    k = (FUSED_SIZES.index(n_fft) + list(WINDOW_CASES).index(wcase)) % len(GRAD_COMBOS)
    for modulated, win_exp, B in (GRAD_COMBOS[k], GRAD_COMBOS[(k + 1) % len(GRAD_COMBOS)]):
        check_istft_gradient(S, 'float32', n_fft, window, wlf(n_fft), hopf(n_fft), _default_N(n_fft, hopf(n_fft)), modulated,
                             win_exp, B, 'fused')


@pytest.mark.parametrize('dtype,n_fft,window,hop,N,modulated,win_exp,B', [
    ('float64', 128, None, 3, 677, True, 1, 2),
    ('float64', 256, 'hann', 64, 1317, False, 2, 0),
    ('float64', 100, 'hann', 12, 537, True, 1, 2),
    ('float64', 101, 'hann', 12, 542, True, 0, 0),
    ('float64', 101, None, 1, 300, False, 1, 2),
    ('float32', 100, 'hann', 12, 537, True, 1, 2),
    ('float32', 101, None, 3, 400, False, 2, 0),
    ('float32', 64, 'hann', 8, 357, True, 1, 2),
])
def test_composed_istft_gradient(S, dtype, n_fft, window, hop, N, modulated, win_exp, B):
    check_istft_gradient(S, dtype, n_fft, window, None, hop, N, modulated, win_exp, B, 'rocfft')


# ------------------------------------------------------------------ 5. ssq_istft_adjoint vs the closed form
def _istft_adjoint_closed_form(g, wa, wa1, n_fft, n_hops, hop, N, modulated, dtype):
    """gSx[k, t] = (c_k / n_fft) rfft_k(win_a[r] u[t hop + r]), the frame rotated, in float64."""
    half = n_fft // 2
    wn = _window_norm(wa1, n_fft, hop, N)
    u = np.zeros(max(N + n_fft - 1, (n_hops - 1) * hop + n_fft))
    d = wn[half:half + N]
    u[half:half + N] = np.where(d > np.finfo(dtype).tiny, g.astype(np.float64) / np.where(d > 0, d, 1.), g)
    fr = np.stack([u[t * hop:t * hop + n_fft] * wa.astype(np.float64) for t in range(n_hops)])
    if modulated:
        fr = np.fft.ifftshift(fr, axes=-1)
    c = np.full(n_fft // 2 + 1, 2.)
    c[0] = 1.
    if n_fft % 2 == 0:
        c[-1] = 1.
    out = (np.fft.rfft(fr, axis=-1) * c / n_fft).T
    out[0] = out[0].real
    if n_fft % 2 == 0:
        out[-1] = out[-1].real
    return out


@pytest.mark.parametrize('dtype,n_fft,hop,N,modulated,win_exp', [
    ('float32', 256, 3, 700, True, 1),
    ('float32', 1024, 128, 3000, False, 2),
    ('float64', 100, 7, 501, True, 0),
])
def test_istft_adjoint_abi_vs_closed_form(S, dtype, n_fft, hop, N, modulated, win_exp):
    import torch
    rng = np.random.default_rng(n_fft)
    n_hops = (N - 1) // hop + 1
    wa, wa1 = _win_powers(S, 'hann', None, n_fft, win_exp, dtype)
    g = rng.standard_normal((2, N))
    gS = S.algos.istft_adjoint_gpu(torch.as_tensor(g, dtype=_tdt(dtype), device=DEV), wa, wa1, n_fft, n_hops, hop,
                                   modulated)
    assert tuple(gS.shape) == (2, n_fft // 2 + 1, n_hops) and gS.dtype == _cdt(dtype)
    gq = g.astype(dtype)
    for b in range(2):
        want = _istft_adjoint_closed_form(gq[b], wa, wa1, n_fft, n_hops, hop, N, modulated, dtype)
        err = relmax(_np(gS[b]).astype(np.complex128), want)
        print("measured: ssq_istft_adjoint", dtype, n_fft, hop, N, modulated, win_exp, b, err)
        assert err <= 20 * TOL[dtype]
    one = S.algos.istft_adjoint_gpu(torch.as_tensor(g[1], dtype=_tdt(dtype), device=DEV), wa, wa1, n_fft, n_hops,
                                    hop, modulated)
    assert torch.equal(torch.view_as_real(one), torch.view_as_real(gS[1]))


# ------------------------------------------------------------------ 6. exact adjoints
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n', [300, 301])
def test_colsum_adjoint_is_exact(S, dtype, n):
    import torch
    A = S.algos
    rng = np.random.default_rng(n)
    B, na = 3, 19
    g = rng.standard_normal((B, n)).astype(dtype)
    d = rng.uniform(0.5, 3, na).astype(dtype)
    for div in (None, d):
        for gi in (g, g[0]):
            gZ = _np(A.colsum_adjoint(torch.as_tensor(gi, device=DEV), na, div))
            want = np.repeat(gi[..., None, :], na, axis=-2)
            if div is not None:
                want = gi[..., None, :] / d[:, None]
            assert gZ.dtype == ('complex64' if dtype == 'float32' else 'complex128')
            assert gZ.shape == want.shape
            assert np.array_equal(gZ.real, want) and not gZ.imag.any()
    # through autograd: colsum_real carries the adjoint
    Z = torch.as_tensor(rng.standard_normal((B, na, n)) + 1j * rng.standard_normal((B, na, n)),
                        dtype=_cdt(dtype), device=DEV).requires_grad_(True)
    out = A.colsum_real(Z, d)
    assert out.grad_fn is not None
    out.backward(torch.as_tensor(g, device=DEV))
    assert np.array_equal(_np(Z.grad).real, g[:, None, :] / d[None, :, None]) and not _np(Z.grad).imag.any()


def _band_adjoint_numpy(g, lo, hi, na, cdtype):
    """float64 mask sum, bands ascending, rounded once."""
    B, K1, n = g.shape
    K = K1 - 1
    i = np.arange(na)[None, :, None]
    acc = np.zeros((B, na, n))
    covered = np.zeros((B, na, n), bool)
    for k in range(K):
        m = (i >= lo[:, k][:, None, :]) & (i <= hi[:, k][:, None, :])
        acc = acc + np.where(m, g[:, k][:, None, :], 0.)
        covered |= m
    acc = np.where(covered, acc, g[:, K][:, None, :])
    return acc.astype(np.float32 if cdtype == 'complex64' else np.float64)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('own', [False, True])
def test_band_adjoint_is_exact(S, dtype, own):
    import torch
    A = S.algos
    rng = np.random.default_rng(5 + own)
    B, na, n, K = 2, 21, 203, 3
    cdt = 'complex64' if dtype == 'float32' else 'complex128'
    cc, cw = _curves(n, K, na, rng, B if own else None)
    cw[..., 1] = cw[..., 0] + 2
    cc[..., 1] = np.clip(cc[..., 0] + 1, 0, na - 1)       # overlapping bands
    cc[..., n // 5, 0] = -1
    upper = np.clip(cc + cw, 0, na)
    lower = np.clip(cc - cw, 0, na)
    upper[cc == -1], lower[cc == -1] = 0, 1
    lo, hi = np.swapaxes(lower, -1, -2), np.swapaxes(np.minimum(upper, na - 1), -1, -2)
    g = rng.standard_normal((B, K + 1, n))
    gZ = _np(A.band_colsum_adjoint(torch.as_tensor(g, device=DEV), lo, hi, na, _cdt(dtype)))
    lob, hib = (lo, hi) if own else (np.broadcast_to(lo, (B,) + lo.shape), np.broadcast_to(hi, (B,) + hi.shape))
    want = _band_adjoint_numpy(g, lob, hib, na, cdt)
    assert gZ.dtype == cdt and np.array_equal(gZ.real, want) and not gZ.imag.any()
    assert (want != g[:, K][:, None, :].astype(want.dtype)).any()
    # through issq_cwt with curves: the same adjoint, scaled by 2 / C_ssq on the host
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    Tx = torch.as_tensor(rng.standard_normal((B, na, n)) + 1j * rng.standard_normal((B, na, n)),
                         dtype=_cdt(dtype), device=DEV).requires_grad_(True)
    xc = S.issq_cwt(Tx, wav, cc=cc, cw=cw)
    assert xc.grad_fn is not None and tuple(xc.shape) == (B, K + 1, n)
    xc.backward(torch.as_tensor(g, device=DEV))
    from ssqueezepy_amd.scales import adm_ssq
    want2 = _band_adjoint_numpy(g * float(2 / adm_ssq(wav)), lob, hib, na, cdt)
    assert np.array_equal(_np(Tx.grad).real, want2) and not _np(Tx.grad).imag.any()


# ------------------------------------------------------------------ 7. end to end
def check_masked_stft_round_trip(S, n_fft, hop, N, B, window='hann'):
    """loss = sum (istft(M * stft(x)) - y)^2: gradients w.r.t. the mask and the signal against the
    torch statements of both transforms."""
    import torch
    dtype, tol = 'float32', TOL['float32']
    rng = np.random.default_rng(17)
    x0 = _x(N, B, dtype, seed=4)
    y = torch.as_tensor(rng.standard_normal(tuple(x0.shape)), dtype=torch.float64, device=DEV)
    n_hops = (N - 1) // hop + 1
    M0 = torch.as_tensor(rng.random((n_fft // 2 + 1, n_hops)) + 0.5, dtype=torch.float64, device=DEV)
    kw = dict(window=window, n_fft=n_fft, hop_len=hop)
    x = x0.clone().requires_grad_(True)
    M = M0.to(torch.float32).requires_grad_(True)
    xr_ = S.istft(M * S.stft(x, dtype=dtype, **kw), N=N, **kw)
    ((xr_ - y.to(torch.float32)) ** 2).sum().backward()

    xs = x0.to(torch.float64).requires_grad_(True)
    Ms = M0.clone().requires_grad_(True)
    win = S.get_window(window, n_fft, n_fft=n_fft, dtype=dtype)
    # (torch_stft of the autograd tests designs the default window; this is its statement for a given one)
    Sr = _torch_stft_window(S, xs, win, n_fft, hop, 'reflect')
    xr, wn = torch_istft(S, Ms * Sr, window, n_fft, None, hop, N, True, 1, dtype)
    assert wn.min() >= 0.5
    ((xr - y) ** 2).sum().backward()
    assert relmax(_np(xr_).astype(np.float64), _np(xr)) <= 10 * tol
    eM = relmax(_np(M.grad).astype(np.float64), _np(Ms.grad))
    ex = relmax(_np(x.grad).astype(np.float64), _np(xs.grad))
    print("measured: masked round trip", n_fft, hop, N, B, "dM", eM, "dx", ex)
    assert eM <= 20 * tol and ex <= 20 * tol


def _torch_stft_window(S, x, win, n_fft, hop, padtype):
    """`torch_stft` of the autograd tests for a given (not the default) window: same pad gather,
    `unfold`, rotation, `rfft`; float64."""
    import torch
    from test_gpu_autograd import _pad_sources
    N = x.shape[-1]
    w = torch.as_tensor(np.fft.ifftshift(win).astype(np.float64), device=x.device)
    src = torch.as_tensor(_pad_sources(S, N, n_fft, padtype), device=x.device)
    xp = torch.where(src >= 0, x[..., src.clamp(min=0)], torch.zeros((), dtype=x.dtype, device=x.device))
    fr = torch.fft.ifftshift(xp.unfold(-1, n_fft, hop), dim=-1)
    return torch.fft.rfft(fr * w, dim=-1).transpose(-1, -2)


@pytest.mark.parametrize('n_fft,hop,N,B', [(256, 64, 1317, 2), (1024, 128, 3001, 0)])
def test_masked_stft_round_trip_gradients(S, n_fft, hop, N, B):
    check_masked_stft_round_trip(S, n_fft, hop, N, B)


def test_torch_stft_window_statement_matches_the_autograd_tests(S):
    """The statement above with the default window is `torch_stft` of tests/test_gpu_autograd.py."""
    import torch
    x = _x(300, 0, 'float32').to(torch.float64)
    win = S.get_window(None, 128, n_fft=128, dtype='float32')
    a = _torch_stft_window(S, x, win, 128, 5, 'reflect')
    b, _ = torch_stft(S, x, 128, 5, None, 'reflect', True, 1., 'float32')
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def check_icwt_cwt_dot_product(S, dtype, scales, l1_norm, B, N=400):
    """icwt(cwt(x)) with x_mean = 0 is linear in x: <J v, g> == <v, J^T g>."""
    import torch
    from ssqueezepy_amd import _cwt
    rng = np.random.default_rng(23)
    wav = S.Wavelet(('gmw', {'dtype': dtype} if l1_norm else {'dtype': dtype, 'norm': 'energy'}))
    kw = dict(scales=scales, nv=8, l1_norm=l1_norm)
    _cwt.clear_plan_cache()

    def J(v):
        Wx, scl = S.cwt(v, wav, **kw)
        return S.icwt(Wx, wav, scales=scl, nv=8, l1_norm=l1_norm, x_mean=0)

    v = _x(N, B, dtype, seed=6)
    with torch.no_grad():
        Jv = J(v)
    assert Jv.grad_fn is None
    g = (Jv.double() + 0.1 * torch.as_tensor(rng.standard_normal(tuple(v.shape)), device=DEV)).to(Jv.dtype)
    x = v.clone().requires_grad_(True)
    out = J(x)
    assert out.grad_fn is not None and torch.equal(out.detach(), Jv)
    out.backward(g)
    lhs = float((Jv.double() * g.double()).sum())
    rhs = float((v.double() * x.grad.double()).sum())
    err = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print("measured: icwt(cwt) dot product", dtype, scales, l1_norm, B, lhs, rhs, err)
    assert err <= 20 * TOL[dtype]
    _cwt.clear_plan_cache()


@pytest.mark.parametrize('B', [0, 2])
@pytest.mark.parametrize('l1_norm', [True, False])
@pytest.mark.parametrize('scales', ['log', 'log-piecewise', 'linear'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_icwt_cwt_dot_product(S, dtype, scales, l1_norm, B):
    check_icwt_cwt_dot_product(S, dtype, scales, l1_norm, B)


def check_issq_chain(S, which, dtype, B, N=300):
    """x.grad through issq(ssq(x)[0]) equals x.grad of the forward alone for gTx = the column-sum
    adjoint of g, bit for bit."""
    import torch
    from ssqueezepy_amd import _cwt
    from ssqueezepy_amd.scales import adm_ssq
    rng = np.random.default_rng(29)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    x0 = _x(N, B, dtype, seed=8)
    g = torch.as_tensor(rng.standard_normal(tuple(x0.shape)), dtype=_tdt(dtype), device=DEV)
    _cwt.clear_plan_cache()
    if which == 'ssq_cwt':
        fwd = lambda x: S.ssq_cwt(x, wav, scales='log', nv=8, gamma=1e-2)[0]
        inv = lambda T: S.issq_cwt(T, wav)
        c = 2 / adm_ssq(wav)
    else:
        fwd = lambda x: S.ssq_stft(x, n_fft=64, hop_len=1, dtype=dtype, gamma=1e-3)[0]
        inv = lambda T: S.issq_stft(T, n_fft=64)
        w = S.get_window(None, 64, n_fft=64)
        c = 2 / w[len(w) // 2]
    x = x0.clone().requires_grad_(True)
    out = inv(fwd(x))
    assert out.grad_fn is not None
    out.backward(g)
    # the host-side scaling's own backward, as torch applies it, then the pinned column-sum adjoint
    from ssqueezepy_amd._inverse import _scale
    probe = torch.zeros_like(g).requires_grad_(True)
    _scale(probe, c).backward(g)
    x2 = x0.clone().requires_grad_(True)
    Tx = fwd(x2)
    gTx = S.algos.colsum_adjoint(probe.grad, Tx.shape[-2])
    Tx.backward(gTx)
    assert torch.equal(x.grad, x2.grad), which
    print("measured: issq chain", which, dtype, B, "equal")
    _cwt.clear_plan_cache()


@pytest.mark.parametrize('B', [0, 2])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('which', ['ssq_cwt', 'ssq_stft'])
def test_issq_chain(S, which, dtype, B):
    check_issq_chain(S, which, dtype, B)


# ------------------------------------------------------------------ 8. nothing asked, nothing changed
def test_nothing_asked_nothing_changed(S):
    import torch
    N = 677
    xn = _signal(N, 2, seed=1).astype('float32')
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    Sx = S.stft(xn, n_fft=128, hop_len=16, window='hann')
    Tx, Wx, _, scl = S.ssq_cwt(xn, wav, nv=8)
    rng = np.random.default_rng(0)
    cc, cw = _curves(N, 2, Tx.shape[-2], rng)
    calls = [
        (Sx, lambda Z: S.istft(Z, 'hann', n_fft=128, hop_len=16, N=N)),
        (Tx, lambda Z: S.issq_cwt(Z, wav)),
        (Tx, lambda Z: S.issq_cwt(Z, wav, cc=cc, cw=cw)),
        (Tx[:, :33], lambda Z: S.issq_stft(Z, n_fft=64)),
        (Tx[:, :33], lambda Z: S.issq_stft(Z, n_fft=64, cc=np.minimum(cc, 32), cw=cw)),
        (Wx, lambda Z: S.icwt(Z, wav, scales=scl, nv=8)),
    ]
    for Z, f in calls:
        Z = Z.detach().contiguous()
        with_grad = f(Z.clone().requires_grad_(True))
        assert with_grad.grad_fn is not None
        plain = f(Z)
        assert isinstance(plain, torch.Tensor) and plain.grad_fn is None and not plain.requires_grad
        assert torch.equal(plain, with_grad.detach())
        with torch.no_grad():
            quiet = f(Z.clone().requires_grad_(True))
        assert quiet.grad_fn is None and torch.equal(quiet, plain)
        out = f(Z.cpu().numpy())
        assert isinstance(out, np.ndarray) and np.array_equal(out, plain.cpu().numpy())
    # icwt(one_int=False): single, no gradient, as before
    W1 = Wx[0].detach().clone().requires_grad_(True)
    x2 = S.icwt(W1, wav, scales=scl, nv=8, one_int=False)
    assert x2.grad_fn is None and x2.dtype == torch.float64
    with pytest.raises(NotImplementedError):
        S.icwt(Wx, wav, scales=scl, nv=8, one_int=False)


# ------------------------------------------------------------------ 9. size
def test_istft_full_size(S):
    """64 signals of 160 000 samples, n_fft 1024, hop 256, 'hann', in one call (Sx 164 MB): signals 0
    and 63 against the float64 statement, one backward through it; and hop 1, one signal, default
    window."""
    import torch
    assert DEV == 'cuda', "full size: a GPU only"
    dtype, tol = 'float32', TOL['float32']
    B, N, n_fft, hop = 64, 160000, 1024, 256
    rng = np.random.default_rng(0)
    x = torch.as_tensor(np.stack([two_chirps(N, b) for b in range(B)]), dtype=torch.float32, device=DEV)
    kw = dict(window='hann', n_fft=n_fft, hop_len=hop)
    with torch.no_grad():
        Sx0 = S.stft(x, dtype=dtype, **kw)
    assert S.algos.istft_algo(dtype, n_fft, Sx0.shape[-1], hop, N) == 'fused'
    Sx = Sx0.clone().requires_grad_(True)
    xr = S.istft(Sx, N=N, **kw)
    assert tuple(xr.shape) == (B, N)
    wgt = torch.as_tensor(rng.random(N) + 0.5, dtype=torch.float64, device=DEV)
    _x_loss(xr, wgt.to(torch.float32)).backward()
    for b in (0, 63):
        Sr = Sx0[b].to(torch.complex128).requires_grad_(True)
        ref, wn = torch_istft(S, Sr, 'hann', n_fft, None, hop, N, True, 1, dtype)
        # (N is a multiple of the hop: two frames instead of four reach the last samples, wn falls to 0.25 there)
        err = relmax(_np(xr[b]).astype(np.float64), _np(ref))
        print("measured: istft full size, signal", b, "wn.min %.3g" % wn.min(), err)
        assert err <= tol
        if b == 63:
            _x_loss(ref, wgt).backward()
            eg = relmax(_np(Sx.grad[b]).astype(np.complex128), _np(Sr.grad))
            print("measured: istft full size gradient, signal 63", eg)
            assert eg <= 20 * tol
    del Sx, Sx0, xr
    with torch.no_grad():
        S1 = S.stft(x[0], dtype=dtype, n_fft=n_fft, hop_len=1)
        assert S.algos.istft_algo(dtype, n_fft, S1.shape[-1], 1, N) == 'fused'
        x1 = S.istft(S1, n_fft=n_fft, hop_len=1, N=N)
        ref, wn = torch_istft(S, S1.to(torch.complex128), None, n_fft, None, 1, N, True, 1, dtype)
    assert wn.min() >= 0.5
    err = relmax(_np(x1).astype(np.float64), _np(ref))
    print("measured: istft full size, hop 1", err)
    assert err <= tol
