# -*- coding: utf-8 -*-
"""What a caller may hand over: views, strides, the lazy-conjugate / lazy-negative bits, base
pointers aligned to no more than an element, other dtypes, gradients in whatever layout the
downstream graph produces -- for every public function that takes a caller's array.

The kernels receive a raw `data_ptr()` and read a dense array there (include/ssq_hip.h, "pointers");
`algos.to_device` is what makes one of whatever arrives. Two assertions per case:

* same values, same result: the call on the odd layout has the bits of the call on the plain tensor
  (`np.array_equal`; the kernels are deterministic and their arithmetic does not depend on where the
  bytes came from). The one documented exception is `Tx` of the fused `ssq_cwt` / `ssq_stft` in the
  default arrival-order mode, compared with `conftest.assert_tx_repeat`. No kernel was found whose
  summation order depends on the base alignment: the only address test in csrc/ (`ssq_colsum_adjoint`,
  csrc/ssq_inverse.hip: ``((uintptr_t)gZ & 15) == 0``) chooses between 16- and 8-byte stores of the
  same values.
* right answer: once per function and dtype an odd layout is compared with the float64 reference the
  suite already uses for that function, at the bound it already asserts there (1e-5 / 1e-12 of the
  largest magnitude for a transform, exact for bins and ordered sums, the golden files' own bounds
  for the inverses).

The signals hold float32-representable values, so that a float64 tensor and a float32 tensor of
them denote the same numbers ("wider_dtype")."""
import os
import numpy as np
import pytest
from conftest import (two_chirps, golden, kernel_inputs, make_ssq_freqs, assert_tx_repeat,
                      assert_tx_vs_oracle)
from test_gpu_autograd import torch_stft, _stft_loss, relmax
from test_gpu_inverse_batched import _win_powers, _curves

pytestmark = pytest.mark.gpu
TOL = {'float32': 1e-5, 'float64': 1e-12}
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ('float32', 'float64')


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def _np(t):
    if isinstance(t, np.ndarray):
        return t
    return t.detach().cpu().numpy()


def _cplx(dtype):
    return 'complex64' if dtype == 'float32' else 'complex128'


def _other(dt):
    return {'float32': 'float64', 'float64': 'float32', 'complex64': 'complex128',
            'complex128': 'complex64'}[str(np.dtype(dt))]


# ---------------------------------------------------------------------------------- the layouts
def plain(values):
    import torch
    return torch.as_tensor(values).to(DEV).clone()


def _holds(t, values):
    """The layout denotes exactly `values` (checked on the host, through torch's own view logic)."""
    import torch
    if isinstance(t, np.ndarray):
        return np.array_equal(t, values)
    return np.array_equal(t.detach().resolve_conj().resolve_neg().cpu().numpy().astype(values.dtype), values)


def real_layouts(values, only=None):
    """(name, array) pairs that hold exactly the real `values` ((N,) or (B, N)) on `DEV`."""
    import torch
    v = np.ascontiguousarray(values)
    tv = torch.as_tensor(v).to(DEV)
    sh, N = v.shape, v.shape[-1]
    out = []
    buf = torch.zeros(v.size + 1, dtype=tv.dtype, device=DEV)
    buf[1:] = tv.reshape(-1)
    out.append(('offset1', buf[1:].view(sh)))
    assert out[-1][1].data_ptr() % 16 != 0, "offset1 is not an offset pointer any more"
    if v.ndim == 1 and N % 2 == 1:
        xb = torch.zeros((3, N), dtype=tv.dtype, device=DEV)
        xb[1] = tv
        out.append(('row_of_odd_batch', xb[1]))
        assert xb[1].data_ptr() % 16 != 0
    big = torch.zeros(sh[:-1] + (2 * N,), dtype=tv.dtype, device=DEV)
    big[..., ::2] = tv
    out.append(('strided', big[..., ::2]))
    rev = np.ascontiguousarray(v[..., ::-1])
    out.append(('reversed', rev[..., ::-1]))                     # NumPy, negative stride
    assert out[-1][1].strides[-1] < 0
    if v.ndim == 2 and (v == v[:1]).all():
        out.append(('expanded', tv[0].expand(sh)))
        assert out[-1][1].stride(0) == 0
    if v.ndim == 2:
        out.append(('fortran_batch', tv.t().contiguous().t()))
        assert out[-1][1].stride() == (1, sh[0])
    out.append(('wider_dtype' if v.dtype == np.float32 else 'narrower_dtype',
                torch.as_tensor(v.astype(_other(v.dtype))).to(DEV)))
    neg = torch.complex(torch.zeros_like(tv), -tv).conj().imag
    assert neg.is_neg()
    out.append(('neg_bit', neg))
    leaf = tv.clone().requires_grad_(True)
    out.append(('requires_grad_view', leaf.view(sh)))
    assert not out[-1][1].is_leaf
    for name, t in out:
        assert _holds(t, v.astype(_other(v.dtype)) if 'dtype' in name else v), name
    return [(n, t) for n, t in out if only is None or n in only]


def complex_layouts(values, only=None, wider=False):
    """(name, tensor) pairs that hold exactly the complex `values` ((rows, n) or (B, rows, n))."""
    import torch
    v = np.ascontiguousarray(values)
    tv = torch.as_tensor(v).to(DEV)
    sh = v.shape
    rows, n = sh[-2:]
    out = [('conj', torch.as_tensor(np.conj(v)).to(DEV).conj())]
    assert out[-1][1].is_conj()
    out.append(('transposed', tv.transpose(-1, -2).contiguous().transpose(-1, -2)))
    assert not out[-1][1].is_contiguous()
    if v.ndim == 2:
        Zb = torch.zeros((3,) + sh, dtype=tv.dtype, device=DEV)
        Zb[1] = tv
        out.append(('batch_slice', Zb[1]))
        if rows * n % 2 == 1 and v.dtype == np.complex64:
            assert Zb[1].data_ptr() % 16 == 8
    else:
        Zb = torch.zeros((sh[0] + 1,) + sh[1:], dtype=tv.dtype, device=DEV)
        Zb[1:] = tv
        out.append(('batch_slice', Zb[1:]))
    big = torch.zeros(sh[:-1] + (n + 2,), dtype=tv.dtype, device=DEV)
    big[..., 1:-1] = tv
    out.append(('col_slice', big[..., 1:-1]))
    big = torch.zeros(sh[:-2] + (2 * rows, n), dtype=tv.dtype, device=DEV)
    big[..., ::2, :] = tv
    out.append(('row_step', big[..., ::2, :]))
    ri = torch.zeros(sh + (4,), dtype=tv.real.dtype, device=DEV)
    ri[..., 0], ri[..., 2] = tv.real, tv.imag
    out.append(('from_real_pair', torch.complex(ri[..., 0], ri[..., 2])))
    if wider:
        out.append(('wider_dtype', torch.as_tensor(v.astype(_other(v.dtype))).to(DEV)))
    ct = torch.as_tensor(np.conj(v)).to(DEV).transpose(-1, -2).contiguous().transpose(-1, -2).conj()
    assert ct.is_conj() and not ct.is_contiguous()
    out.append(('conj_transposed', ct))
    for name, t in out:
        assert _holds(t, v.astype(_other(v.dtype)) if 'dtype' in name else v), name
    return [(n_, t) for n_, t in out if only is None or n_ in only]


def check_layouts(f, layouts, want, tx=(), what='', want_grad=None):
    """`f(layout)` (a tuple of arrays) has the bits of `want` = `f(plain)`; the outputs listed in `tx`
    are a fused transform's `Tx` in arrival order (`assert_tx_repeat`). `want_grad`: `f` of the plain
    tensor that requires grad, where that call takes another kernel than the one without a gradient
    (`ssq_stft` / `ssq_cwt` keep `dWx` for the backward: the ordered reassignment)."""
    want_plain = [_np(a) for a in want]
    want_grad = want_plain if want_grad is None else [_np(a) for a in want_grad]
    res = None
    for name, t in layouts:
        want = want_grad if name == 'requires_grad_view' else want_plain
        res = [_np(a) for a in f(t)]
        assert len(res) == len(want)
        for i, (a, b) in enumerate(zip(res, want)):
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name, i, a.shape, a.dtype, b.dtype)
            if i in tx:
                assert_tx_repeat(a, b, what=(what, name, i))
            else:
                assert np.array_equal(a, b), (what, name, i, float(np.abs(a - b).max()))
    return res


def _sig(N, B, dtype, seed=1, same_rows=False):
    x = np.stack([two_chirps(N, seed + (0 if same_rows else b)) for b in range(max(B, 1))])
    x = x.astype('float32').astype(dtype)              # float32-representable in either dtype
    return x if B else x[0]


# ------------------------------------------------------------------------- 1. forward transforms
# (dtype, n_fft, hop, N, route, generic switch): hop 1, n_fft // 4, and 37 (a partial last workgroup)
STFT_CASES = [
    ('float32', 128, 1, 301, 'fused', False),
    ('float32', 128, 32, 1501, 'fused', False),
    ('float32', 1024, 37, 3001, 'fused', False),
    ('float32', 598, 37, 1501, 'fused-mixed-radix', False),
    ('float32', 256, 64, 1501, 'rocfft', True),
    ('float64', 128, 32, 1501, 'rocfft', False),
    ('float64', 100, 1, 301, 'rocfft', False),
]


def _last_stft_plan():
    from ssqueezepy_amd import _stft
    return list(_stft._PLAN_CACHE.values())[-1]


@pytest.mark.parametrize('case', STFT_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_stft_and_ssq_stft_input_layouts(S, orc, case, monkeypatch):
    """`stft` (with its derivative) over every layout of a single signal, `ssq_stft` over every
    layout of a batch, on each route the plan can choose (asserted); then an offset-pointer signal
    against the oracle: Sx, dSx at 1e-5 / 1e-12, Tx (dSx kept: the ordered kernel) exactly against
    the oracle's reassignment of the device's own Sx, dSx."""
    from pipeline import oracle_ssq_stft
    from ssqueezepy_amd import _stft
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    dtype, n_fft, hop, N, route, generic = case
    if generic:
        monkeypatch.setenv('SSQ_DEBUG_STFT_GENERIC', '1')
    _stft._PLAN_CACHE.clear()
    kw = dict(n_fft=n_fft, hop_len=hop, dtype=dtype)
    x = _sig(N, 0, dtype)
    f = lambda t: S.stft(t, derivative=True, **kw)
    want = f(plain(x))
    assert _last_stft_plan().algo == route
    res = check_layouts(f, real_layouts(x), want, what='stft')
    f0 = lambda t: (S.stft(t, **kw),)
    check_layouts(f0, real_layouts(x, only=('offset1', 'strided', 'neg_bit')), f0(plain(x)), what='stft, no derivative')

    xb = _sig(N, 3, dtype, same_rows=True)
    fb = lambda t: S.ssq_stft(t, **kw)[:2]
    wantb = fb(plain(xb))
    assert _last_stft_plan().algo == route
    check_layouts(fb, real_layouts(xb), wantb, tx=(0,), what='ssq_stft', want_grad=fb(plain(xb).requires_grad_(True)))

    off = real_layouts(x, only=('offset1',))[0][1]
    Tx, Sx, sf, Sfs, dSx = [_np(a) for a in S.ssq_stft(off, get_dWx=True, **kw)]
    ro = oracle_ssq_stft(orc, x.astype(np.float64), dtype, n_fft=n_fft, hop_len=hop)
    assert relmax(Sx, ro['Sx']) <= TOL[dtype] and relmax(dSx, ro['dSx']) <= TOL[dtype]
    assert relmax(_np(res[0]), ro['Sx']) <= TOL[dtype]
    _, p = ssq_grid_params(Sfs, False)
    ref = orc.ssqueeze(Sx, dSx, 'linear', p, Sfs[1] - Sfs[0], ro['gamma'], False, Sfs=Sfs, typing=0)
    assert np.array_equal(Tx, ref)
    _stft._PLAN_CACHE.clear()


# (dtype, scales, nv, N, tiles): the column-tile path, the block path (SSQ_CWT_TILES=0), float64
CWT_CASES = [
    ('float32', 'log', 16, 2501, True),
    ('float32', 'log', 16, 2501, False),
    ('float32', 'log-piecewise', 8, 601, None),
    ('float64', 'log', 8, 601, None),
]


@pytest.mark.parametrize('case', CWT_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_cwt_and_ssq_cwt_input_layouts(S, orc, case, monkeypatch):
    """`cwt` with and without `derivative` over every layout of a single signal, `ssq_cwt` over
    every layout of a batch, on the column-tile path and on the block path (what executed is
    asserted: `plan.tiles_done()`); then an offset-pointer signal against the oracle: Wx, dWx at
    1e-5 / 1e-12, Tx against the oracle's reassignment of the device's own Wx, dWx
    (`assert_tx_vs_oracle`)."""
    from pipeline import oracle_ssq_cwt, GRIDNAME
    from ssqueezepy_amd import _cwt
    dtype, scales, nv, N, tiles = case
    if tiles is True and os.environ.get('SSQ_CWT_TILES', '') == '0':
        pytest.skip('the column-tile path is switched off (SSQ_CWT_TILES=0)')
    if tiles is False:
        monkeypatch.setenv('SSQ_CWT_TILES', '0')
    _cwt.clear_plan_cache()
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    kw = dict(scales=scales, nv=nv)
    x = _sig(N, 0, dtype)
    f = lambda t: (lambda r: (r[0], r[2]))(S.cwt(t, wav, derivative=True, **kw))
    check_layouts(f, real_layouts(x), f(plain(x)), what='cwt')
    f0 = lambda t: S.cwt(t, wav, **kw)[:1]
    check_layouts(f0, real_layouts(x, only=('offset1', 'strided', 'neg_bit')), f0(plain(x)), what='cwt, no derivative')

    _cwt.clear_plan_cache()
    xb = _sig(N, 3, dtype, same_rows=True)
    fb = lambda t: S.ssq_cwt(t, wav, **kw)[:2]
    wantb = fb(plain(xb))
    plan = list(_cwt._PLAN_CACHE.values())[-1]
    if tiles is True:
        assert plan.tile_rows > 0.5 * plan.na and plan.tiles_done() == 3 * plan.tiles_per_signal(N)
    elif tiles is False:
        assert plan.tile_rows == 0
    check_layouts(fb, real_layouts(xb), wantb, tx=(0,), what='ssq_cwt', want_grad=fb(plain(xb).requires_grad_(True)))

    off = real_layouts(x, only=('offset1',))[0][1]
    Tx, Wx, sf, sc, dWx = [_np(a) for a in S.ssq_cwt(off, wav, get_dWx=True, **kw)]
    r = oracle_ssq_cwt(orc, x.astype(np.float64), dtype, scales=scales, nv=nv)
    assert relmax(Wx, r['Wx']) <= TOL[dtype] and relmax(dWx, r['dWx']) <= TOL[dtype]
    assert np.array_equal(sf, r['ssq_freqs'])
    ref = orc.ssqueeze(Wx, dWx, GRIDNAME[r['grid']], r['params'], r['const'], r['gamma'], True, typing=0)
    assert_tx_vs_oracle(Tx, ref)
    _cwt.clear_plan_cache()


def test_float16_and_int32_signals(S):
    """float16 and int32 signals are accepted and converted: the transforms of an integer-valued
    signal equal those of the float32 tensor of the same values."""
    import torch
    N = 601
    xi = np.rint(8 * two_chirps(N, 2)).astype(np.int32)
    want32 = plain(xi.astype(np.float32))
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    fs = {'stft': lambda t: (S.stft(t, n_fft=128, hop_len=32),),
          'ssq_stft': lambda t: S.ssq_stft(t, n_fft=128, hop_len=32, get_dWx=True)[:2],
          'cwt': lambda t: S.cwt(t, wav, nv=8)[:1],
          'ssq_cwt': lambda t: S.ssq_cwt(t, wav, nv=8)[:2],
          'buffer': lambda t: (S.algos.buffer(t, 64, 48),)}
    for name, f in fs.items():
        lay = [('int32', torch.as_tensor(xi).to(DEV)), ('float16', torch.as_tensor(xi.astype(np.float16)).to(DEV)),
               ('int32_strided', torch.as_tensor(np.repeat(xi, 2)).to(DEV)[::2]), ('numpy_int32', xi)]
        assert _holds(lay[1][1], xi.astype(np.float16))
        check_layouts(f, lay, f(want32), tx=(0,) if name == 'ssq_cwt' else (), what=name)


@pytest.mark.parametrize('dtype', DTYPES)
def test_buffer_pad_replace_input_layouts(S, orc, dtype):
    """`algos.buffer`, `pad_signal_gpu` (real layouts, single and batched) and `replace_under_abs`
    (complex layouts of `ref`): the bits of the plain call, which are the oracle's / NumPy's."""
    A = S.algos
    x = _sig(1001, 0, dtype)
    xb = _sig(1001, 3, dtype, same_rows=True)
    for v in (x, xb):
        f = lambda t: (A.buffer(t, 100, 60, True), A.pad_signal_gpu(t, 23, 18, 'reflect'),
                       A.pad_signal_gpu(t, 0, 7, 'wrap'))
        lays = [(n, t) for n, t in real_layouts(v) if 'dtype' not in n]
        res = check_layouts(f, lays, f(plain(v)), what='buffer/pad')
    assert np.array_equal(res[0][1], orc.buffer(xb[1], 100, 60, True))
    assert np.array_equal(res[1], np.pad(xb, ((0, 0), (23, 18)), mode='reflect'))
    na, n = 37, 75
    Wx, dWx, w, *_ = kernel_inputs(dtype, na, n)
    want = np.where(np.abs(Wx) < 1.5, np.inf, w).astype(dtype)
    for name, t in complex_layouts(Wx):
        wt = plain(w)
        A.replace_under_abs(wt, t, 1.5, np.inf)
        assert np.array_equal(_np(wt), want), name
    # the array modified in place must be dense: a view is refused, not written through its base pointer
    wv = plain(np.repeat(w, 2, axis=1))[:, ::2]
    with pytest.raises(TypeError):
        A.replace_under_abs(wv, Wx, 1.5, np.inf)


# ------------------------------------------------------------------ 2. the two-step reassignment
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('batched', [False, True], ids=['single', 'batch'])
def test_reassignment_input_layouts(S, orc, dtype, batched):
    """`ssqueeze_fast`, `indexed_sum_onfly`, `phase_cwt_gpu`, `phase_stft_gpu`, the public `ssqueeze`
    (`dWx=` and `w=` forms), `phase_cwt` and `phase_stft` over every complex layout of `Wx` and of
    `dWx` (a complex128 `dWx` for complex64 data is converted), and real layouts of `w`. The plain
    result is the oracle's, bin for bin and sum for sum (37 x 75: odd rows * n, so `Zb[1]` starts
    8 bytes off a 16-byte boundary)."""
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    A = S.algos
    na, n, gamma = 37, 75, 1e-2
    Wx, dWx, w, winf, Sfs, _ = kernel_inputs(dtype, na, n)
    if batched:
        Wx, dWx, winf = (np.stack([a, a[::-1], 2 * a]) for a in (Wx, dWx, winf))
    sf = make_ssq_freqs(na, 'log')
    _, p = ssq_grid_params(sf, True)
    _, pl = ssq_grid_params(Sfs, False)
    const = np.log(2) / 32
    dS = Sfs[1] - Sfs[0]
    pW, pD = plain(Wx), plain(dWx)

    def f_W(t, d=None):
        d = pD if d is None else d
        Tx, k = A.ssqueeze_fast(t, d, sf, const, True, True, gamma, get_k=True)
        Ts = A.ssqueeze_fast(t, d, Sfs, dS, False, False, gamma, Sfs=Sfs)
        return (Tx, k, Ts, A.phase_cwt_gpu(t, d, gamma), A.phase_stft_gpu(t, d, Sfs, gamma),
                S.ssqueeze(t, ssq_freqs=Sfs, Sfs=Sfs, dWx=d, gamma=gamma, transform='stft')[0],
                S.phase_cwt(t, d, gamma=gamma), S.phase_stft(t, d, Sfs, gamma=gamma),
                A.indexed_sum_onfly(t, plain(winf), Sfs, dS, False, False),
                S.ssqueeze(t, w=plain(winf), ssq_freqs=Sfs, transform='stft')[0])
    want = f_W(pW)
    res = check_layouts(f_W, complex_layouts(Wx), want, what='Wx')
    check_layouts(lambda d: f_W(pW, d)[:8], complex_layouts(dWx, wider=(dtype == 'float32')), want[:8], what='dWx')
    fw = lambda t: (A.indexed_sum_onfly(pW, t, Sfs, dS, False, False),
                    S.ssqueeze(pW, w=t, ssq_freqs=Sfs, transform='stft')[0])
    w2 = winf.reshape(-1, n)
    lays = [(nm, t.reshape(winf.shape) if not isinstance(t, np.ndarray) else t.reshape(winf.shape))
            for nm, t in real_layouts(w2, only=('offset1', 'strided', 'fortran_batch', 'wider_dtype'))]
    check_layouts(fw, lays, want[8:], what='w')

    # right answer: the last layout's results (conj on top of transposed) against the oracle
    first = lambda a: a[0] if batched else a
    W0, D0 = first(Wx), first(dWx)
    ref, kref = orc.ssqueeze(W0, D0, 'log', p, const, gamma, True, typing=0, get_k=True)
    assert np.array_equal(first(res[0]), ref) and np.array_equal(first(res[1]), kref)
    refs = orc.ssqueeze(W0, D0, 'linear', pl, dS, gamma, False, Sfs=Sfs, typing=0)
    assert np.array_equal(first(res[2]), refs) and np.array_equal(first(res[5]), refs)
    assert np.array_equal(first(res[3]), orc.phase_cwt(W0, D0, gamma, typing=0))
    assert np.array_equal(first(res[6]), orc.phase_cwt(W0, D0, gamma, typing=0))
    assert np.array_equal(first(res[4]), orc.phase_stft(W0, D0, Sfs, gamma, typing=0))
    assert np.array_equal(first(res[7]), orc.phase_stft(W0, D0, Sfs, gamma, typing=0))
    refi = orc.indexed_sum(W0, first(winf), 'linear', pl, dS, False, typing=0)
    assert np.array_equal(first(res[8]), refi) and np.array_equal(first(res[9]), refi)


def _bad_outs(Wx):
    """`out=` arguments that must be refused, each on a storage at least as large as a correct one."""
    import torch
    sh = tuple(Wx.shape)
    bad = {'transposed': torch.zeros(sh[:-2] + (sh[-1], sh[-2]), dtype=Wx.dtype, device=DEV).transpose(-1, -2),
           'wider dtype': torch.zeros(sh, dtype=torch.complex128 if Wx.dtype == torch.complex64 else torch.float64,
                                      device=DEV),
           'larger shape': torch.zeros(sh[:-1] + (sh[-1] + 1,), dtype=Wx.dtype, device=DEV),
           'strided': torch.zeros(sh[:-1] + (2 * sh[-1],), dtype=Wx.dtype, device=DEV)[..., ::2]}
    if Wx.dtype == torch.complex128:
        bad['wider dtype'] = torch.zeros(sh + (2,), dtype=torch.complex128, device=DEV)
        bad['other dtype'] = torch.zeros(sh + (2,), dtype=torch.float64, device=DEV)
    if DEV == 'cuda':
        bad['host'] = torch.zeros(sh, dtype=Wx.dtype)
    return bad


@pytest.mark.parametrize('dtype', DTYPES)
def test_out_arguments_are_validated(S, dtype):
    """`ssqueeze_fast`, `indexed_sum_onfly` and `ssqueeze_adjoint` write `out` through its raw
    pointer: a non-contiguous `out`, one of another dtype or shape, or one on the host raises
    ValueError before anything is launched (the refused tensor is untouched); a correct `out` is
    filled and returned."""
    import torch
    A = S.algos
    na, n, gamma = 12, 20, 1e-2
    Wx, dWx, w, winf, Sfs, _ = kernel_inputs(dtype, na, n)
    pW, pD, pw = plain(Wx), plain(dWx), plain(winf)
    dS = Sfs[1] - Sfs[0]
    calls = {'ssqueeze_fast': lambda out: A.ssqueeze_fast(pW, pD, Sfs, dS, False, False, gamma, out=out, Sfs=Sfs),
             'indexed_sum_onfly': lambda out: A.indexed_sum_onfly(pW, pw, Sfs, dS, False, False, out=out),
             'ssqueeze_adjoint': lambda out: A.ssqueeze_adjoint(pW, pD, pW, Sfs, dS, False, False, gamma, Sfs=Sfs,
                                                                out=out)}
    for name, call in calls.items():
        for kind, out in _bad_outs(pW).items():
            with pytest.raises(ValueError):
                call(out)
            assert not bool(out.cpu().to(torch.complex128).abs().sum()), (name, kind, "written before the refusal")
        good = torch.zeros_like(pW)
        assert call(good) is good and torch.equal(good, call(None)), name


# ----------------------------------------------------------------------------------- 3. inverses
@pytest.mark.parametrize('dtype', DTYPES)
def test_inverse_cwt_input_layouts(S, dtype):
    """`icwt` (one_int True: 'log' and 'log-piecewise', L2 norm; one_int False), `issq_cwt` (with and
    without curves), `trigdiff` and `colsum_real` over the complex layouts, on the reference's own
    transforms (tests/golden): exact where test_gpu_inverse.py compares exactly, its bounds elsewhere."""
    g, g2, gt = golden('inverse'), golden('icwt2'), golden('trigdiff')
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    x = g[f'x/{dtype}']
    for st in ('log', 'log-piecewise'):
        pre = f'{dtype}/{st}'
        Wx, Tx, sc = g['Wx/' + pre], g['Tx/' + pre], g['scales/' + pre]
        f = lambda t: (S.icwt(t, wav, scales=sc, nv=8, x_mean=x.mean()), S.issq_cwt(t, wav))
        res = check_layouts(f, complex_layouts(Wx), f(plain(Wx)), what='icwt ' + st)
        assert np.array_equal(res[0], g['icwt/' + pre])
        fs = lambda t: (S.issq_cwt(t, wav),)
        res = check_layouts(fs, complex_layouts(Tx, only=('conj', 'col_slice', 'conj_transposed')), fs(plain(Tx)))
        assert np.array_equal(res[0], g['issq/' + pre])
    wav2 = S.Wavelet(('gmw', {'dtype': dtype, 'norm': 'energy'}))
    Wl, scl = g[f'Wx/{dtype}/l2'], g[f'scales/{dtype}/l2']
    f = lambda t: (S.icwt(t, wav2, scales=scl, nv=8, l1_norm=False),)
    res = check_layouts(f, complex_layouts(Wl, only=('conj', 'batch_slice', 'row_step')), f(plain(Wl)))
    assert np.array_equal(res[0], g[f'icwt/{dtype}/l2'])
    Tl, cc, cw = g[f'Tx/{dtype}/log'], g[f'cc/{dtype}'], g[f'cw/{dtype}']
    f = lambda t: (S.issq_cwt(t, wav, cc, cw),)
    res = check_layouts(f, complex_layouts(Tl), f(plain(Tl)), what='issq_cwt curves')
    assert np.array_equal(res[0], g[f'issq_comp/{dtype}'])
    Wb, scb = g[f'Wxb/{dtype}'], g[f'scb/{dtype}']
    f = lambda t: (S.icwt(t, wav, scales=scb, nv=8),)
    res = check_layouts(f, complex_layouts(Wb), f(plain(Wb)), what='icwt batch')
    assert np.array_equal(res[0], g[f'icwt_b/{dtype}'])

    x2 = g2['x']
    tol = 2e-5 if dtype == 'float32' else 1e-11                  # (test_icwt_double_integral's)
    for st in ('log', 'log-piecewise'):
        Wx, sc, ref = g2[f'Wx/{dtype}/{st}'], g2[f'sc/{dtype}/{st}'], g2[f'icwt2/{dtype}/{st}']
        f = lambda t: (S.icwt(t, wav, scales=sc, nv=8, one_int=False, x_len=len(x2), x_mean=x2.mean()),)
        res = check_layouts(f, complex_layouts(Wx), f(plain(Wx)), what='icwt2 ' + st)
        assert relmax(res[0], ref) <= tol

    Wx, Wp = gt[f'Wx/{dtype}'], gt[f'Wp/{dtype}']
    N = Wx.shape[-1]
    for name, v, kw in (('pad_N', Wx, dict(fs=2.0, padtype='reflect', N=N)),
                        ('rpadded', Wp, dict(fs=0.5, rpadded=True, N=N))):
        f = lambda t: (S.trigdiff(t, **kw),)
        res = check_layouts(f, complex_layouts(v), f(plain(v)), what='trigdiff ' + name)
        assert relmax(res[0], gt[f'{name}/{dtype}']) <= TOL[dtype]

    na, n = 19, 301
    rng = np.random.default_rng(3)
    Z = (rng.standard_normal((2, na, n)) + 1j * rng.standard_normal((2, na, n))).astype(_cplx(dtype))
    d = rng.uniform(1, 2, na).astype(dtype)
    f = lambda t: (S.algos.colsum_real(t), S.algos.colsum_real(t, d))
    for v in (Z, Z[0]):
        res = check_layouts(f, complex_layouts(v), f(plain(v)), what='colsum_real')
        assert np.array_equal(res[0], v.real.sum(axis=-2))
        assert np.array_equal(res[1], (v.real / d[:, None]).sum(axis=-2))
    cc, cw = _curves(n, 2, na, rng)
    upper, lower = np.clip(cc + cw, 0, na), np.clip(cc - cw, 0, na)
    upper[cc == -1], lower[cc == -1] = 0, 1
    lo, hi = lower.T, np.minimum(upper, na - 1).T
    f = lambda t: (S.algos.band_colsum(t, lo, hi),)
    res = check_layouts(f, complex_layouts(Z), f(plain(Z)), what='band_colsum')
    want = np.zeros((2, 3, n))
    for b in range(2):
        for j in range(n):
            covered = np.zeros(na, bool)
            for k in range(2):
                acc = 0.0
                for i in range(lo[k, j], min(hi[k, j], na - 1) + 1):
                    acc += float(Z[b, i, j].real)
                    covered[i] = True
                want[b, k, j] = acc
            acc = Z.real.dtype.type(0)
            for i in np.nonzero(~covered)[0]:
                acc = acc + Z[b, i, j].real
            want[b, 2, j] = acc
    assert np.array_equal(res[0], want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_inverse_stft_input_layouts(S, dtype):
    """`istft` on the fused and on the composed route (asserted through `algos.istft_algo`) and
    `issq_stft` with and without curves over the complex layouts; against the reference's outputs
    (tests/golden/inverse.npz) at test_gpu_inverse.py's bounds."""
    g = golden('inverse')
    # (N, n_fft, hop, win_len, window, modulated, win_exp)
    for (N, n_fft, hop, win_len, win, mod, we) in ((1024, 128, 16, None, None, True, 1),
                                                   (1000, 100, 10, 80, 'hann', True, 1),
                                                   (300, 64, 1, None, None, True, 2)):
        pre = f'{dtype}/{N}/{n_fft}/{hop}'
        Sx, ref = g['Sx/' + pre], g['istft/' + pre]
        algo = S.algos.istft_algo(dtype, n_fft, Sx.shape[-1], hop, N)
        assert algo == ('fused' if (dtype, n_fft) == ('float32', 128) else 'rocfft')
        f = lambda t: (S.istft(t, win, n_fft=n_fft, win_len=win_len, hop_len=hop, N=N, modulated=mod, win_exp=we),)
        for v in (Sx, np.stack([Sx, 2 * Sx])):
            res = check_layouts(f, complex_layouts(v), f(plain(v)), what=('istft', pre, algo))
        assert relmax(res[0][0], ref) <= TOL[dtype]
    Tx = g[f'Txs/{dtype}']
    f = lambda t: (S.issq_stft(t, n_fft=64, hop_len=1),
                   S.issq_stft(t, cc=g[f'ccs/{dtype}'], cw=g[f'cws/{dtype}'], n_fft=64, hop_len=1))
    res = check_layouts(f, complex_layouts(Tx), f(plain(Tx)), what='issq_stft')
    assert np.array_equal(res[0], g[f'issq_stft/{dtype}'])
    assert np.array_equal(res[1], g[f'issq_stft_comp/{dtype}'])


@pytest.mark.parametrize('cdtype', ['complex64', 'complex128', 'float32'])
def test_extract_ridges_input_layouts(S, orc, cdtype):
    """`extract_ridges`, single and batched, over the layouts; against the oracle's tracking at
    test_gpu_ridges.py's criterion (99 % of the indices, the dominant ridge everywhere)."""
    from test_gpu_ridges import _random_tf
    rng = np.random.default_rng(4)
    na, n = 65, 385
    Tf = np.stack([_random_tf(rng, na, n, 'complex128') for _ in range(2)])
    Tf = np.abs(Tf).astype(cdtype) if cdtype == 'float32' else Tf.astype('complex64').astype(cdtype)
    scales = np.exp(np.linspace(-0.3, 6.2, na))
    kw = dict(penalty=2.0, n_ridges=2, bw=4, transform='cwt', get_params=True)
    f = lambda t: S.extract_ridges(t, scales, **kw)
    for v in (Tf, Tf[1]):
        if cdtype == 'float32':
            lays = [(nm, t.reshape(v.shape)) for nm, t in real_layouts(v.reshape(-1, n),
                    only=('offset1', 'strided', 'fortran_batch', 'neg_bit'))]
        else:
            lays = complex_layouts(v)
        res = check_layouts(f, lays, f(plain(v)), what='extract_ridges')
    ri, rf, re = orc.extract_ridges(Tf[1], scales, **kw)
    same = res[0] == ri
    assert same.mean() >= 0.99 and same[:, 0].all()
    assert np.array_equal(res[1][same], rf[same])


# ---------------------------------------------------------------------------------- 4. gradients
def _w(shape, seed, dtype='float64', cplx=False):
    import torch
    rng = np.random.default_rng(seed)
    v = rng.random(shape) + 0.5
    if cplx:
        v = v + 1j * (rng.random(shape) - 0.5)
    return torch.as_tensor(v.astype(('complex128' if cplx else 'float64') if dtype == 'float64'
                                    else ('complex64' if cplx else 'float32'))).to(DEV)


def _to64(o):
    import torch
    return o.to(torch.complex128 if o.is_complex() else torch.float64)


def _mag2(o):
    return o.real ** 2 + o.imag ** 2 if o.is_complex() else o ** 2


# downstream ops of a (B, rows, n) / (B, N) output that hand the backward an upstream gradient in
# an odd layout: stride 0, an offset zero-filled one, a transposed one, a conj-bit one, a float64
# one for float32 outputs
LOSSES = {
    'sum': lambda o: (o.real if o.is_complex() else o).sum(),
    'offset': lambda o: o[..., 3:].abs().sum(),
    'transpose': lambda o: (_mag2(o.transpose(-1, -2).reshape(o.shape[-1], -1))
                            * _w((o.shape[-1], 1), 1, str(o.real.dtype)[6:])).sum(),
    'conj': lambda o: ((o * (0.5 - 2j)).conj() * _w(o.shape, 2, str(o.real.dtype)[6:], True)).imag.sum(),
    'float64': lambda o: (_mag2(_to64(o)) * _w(o.shape, 3)).sum(),
}


def check_incoming_gradient_layouts(f, leaf_values, what):
    """The gradient at the leaf from `loss(f(leaf)).backward()` -- the upstream gradient in the
    layout autograd hands over -- has the bits of the one from the same upstream gradient made a
    plain contiguous tensor first."""
    import torch
    seen = set()
    for kind, loss in LOSSES.items():
        x = plain(leaf_values).requires_grad_(True)
        out = f(x)
        assert out.grad_fn is not None, what
        (g,) = torch.autograd.grad(loss(out), x, retain_graph=True)
        o = out.detach().clone().requires_grad_(True)
        (G,) = torch.autograd.grad(loss(o), o)
        seen.add((G.is_conj(), G.is_contiguous(), G.dtype == out.dtype))
        Gp = G.to(out.dtype).resolve_conj().contiguous().clone()
        (gp,) = torch.autograd.grad(out, x, grad_outputs=Gp)
        assert g.dtype == x.dtype and g.shape == x.shape
        assert float(gp.abs().max()) > 0
        assert torch.equal(torch.view_as_real(g) if g.is_complex() else g,
                           torch.view_as_real(gp) if gp.is_complex() else gp), (what, kind)
    return seen


@pytest.mark.parametrize('dtype', DTYPES)
def test_incoming_gradient_layouts_forward_transforms(S, dtype):
    """Backward of `stft`, `ssq_stft`, `cwt` and `ssq_cwt` (batched; `Tx` and the transform stacked, so
    that each receives a slice of one gradient) under the downstream ops of `LOSSES`."""
    import torch
    N = 501
    x = _sig(N, 2, dtype, seed=3)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    n_fft = 128 if dtype == 'float32' else 100
    fs = {'stft': lambda t: torch.stack(S.stft(t, n_fft=n_fft, hop_len=8, derivative=True, dtype=dtype)),
          'ssq_stft': lambda t: torch.stack(S.ssq_stft(t, n_fft=n_fft, hop_len=8, dtype=dtype, gamma=1e-3)[:2]),
          'cwt': lambda t: S.cwt(t, wav, scales='log', nv=8)[0],
          'ssq_cwt': lambda t: torch.stack(S.ssq_cwt(t, wav, scales='log', nv=8, gamma=1e-2)[:2])}
    for name, f in fs.items():
        check_incoming_gradient_layouts(f, x, name)


@pytest.mark.parametrize('dtype', DTYPES)
def test_incoming_gradient_layouts_inverses(S, dtype):
    """Backward of `istft` (fused route for float32, composed for float64), `issq_stft`, `issq_cwt`
    (with and without curves) and `icwt(one_int=True)` under the downstream ops of `LOSSES`."""
    rng = np.random.default_rng(6)
    N, n_fft, hop = 677, 128, 16
    n_hops = (N - 1) // hop + 1
    assert S.algos.istft_algo(dtype, n_fft, n_hops, hop, N) == ('fused' if dtype == 'float32' else 'rocfft')
    cx = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(_cplx(dtype))
    Sx, Tx = cx(2, n_fft // 2 + 1, n_hops), cx(2, 33, 300)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    cc, cw = _curves(300, 2, 33, rng)
    sc = S.process_scales('log', 300, wav, nv=4)
    Wx = cx(2, len(sc), 300)
    check_incoming_gradient_layouts(lambda t: S.istft(t, 'hann', n_fft=n_fft, hop_len=hop, N=N), Sx, 'istft')
    check_incoming_gradient_layouts(lambda t: S.issq_stft(t, n_fft=64), Tx, 'issq_stft')
    check_incoming_gradient_layouts(lambda t: S.issq_cwt(t, wav), Tx, 'issq_cwt')
    check_incoming_gradient_layouts(lambda t: S.issq_cwt(t, wav, cc=cc, cw=cw), Tx, 'issq_cwt curves')
    check_incoming_gradient_layouts(lambda t: S.icwt(t, wav, scales=sc, nv=4), Wx, 'icwt')


@pytest.mark.parametrize('dtype', DTYPES)
def test_adjoint_entry_points_gradient_layouts(S, dtype):
    """`StftPlan.adjoint`, `algos.ssqueeze_adjoint` (complex gradients: conj, transposed, offset, ...),
    `colsum_adjoint`, `band_colsum_adjoint`, `istft_adjoint_gpu` (real gradients: offset1, strided,
    expanded, column-major) called directly: the bits of the call on the plain gradient."""
    import torch
    from ssqueezepy_amd import _stft
    A = S.algos
    rng = np.random.default_rng(8)
    cx = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(_cplx(dtype))
    N, n_fft, hop = 501, 128 if dtype == 'float32' else 100, 8
    w0, dw0 = S.get_window(None, n_fft, n_fft, derivative=True, dtype=dtype)
    plan = _stft.StftPlan(N, n_fft, hop, w0, dw0, 1., 'reflect', True, dtype, max_batch=2)
    assert plan.algo == ('fused' if dtype == 'float32' else 'rocfft')
    gS, gD = cx(2, plan.rows, plan.n_hops), cx(2, plan.rows, plan.n_hops)
    pS, pD = plain(gS), plain(gD)
    check_layouts(lambda t: (plan.adjoint(t, None), plan.adjoint(t, pD), plan.adjoint(pS, t)),
                  complex_layouts(gS, wider=(dtype == 'float32')),
                  (plan.adjoint(pS, None), plan.adjoint(pS, pD), plan.adjoint(pS, pS)), what='StftPlan.adjoint')

    na, n, gamma = 37, 75, 1e-2
    Wx, dWx, w, winf, Sfs, _ = kernel_inputs(dtype, na, n)
    G = cx(na, n)
    sf = make_ssq_freqs(na, 'log')
    fa = lambda W, D, g: (A.ssqueeze_adjoint(W, D, g, sf, np.log(2) / 32, True, True, gamma),)
    want = fa(plain(Wx), plain(dWx), plain(G))
    check_layouts(lambda t: fa(plain(Wx), plain(dWx), t), complex_layouts(G, wider=(dtype == 'float32')), want)
    check_layouts(lambda t: fa(t, plain(dWx), plain(G)), complex_layouts(Wx), want)
    check_layouts(lambda t: fa(plain(Wx), t, plain(G)), complex_layouts(dWx), want)

    g1 = _sig(301, 3, dtype, seed=2, same_rows=True)
    d = rng.uniform(0.5, 3, 19).astype(dtype)
    lays = [(nm, t) for nm, t in real_layouts(g1) if 'dtype' not in nm]
    fc = lambda t: (A.colsum_adjoint(t, 19), A.colsum_adjoint(t, 19, d))
    res = check_layouts(fc, lays, fc(plain(g1)), what='colsum_adjoint')
    assert np.array_equal(res[1].real, g1[:, None, :] / d[None, :, None]) and not res[1].imag.any()
    n_hops = (301 - 1) // 4 + 1
    wa, wa1 = _win_powers(S, 'hann', None, 64, 1, dtype)
    fi = lambda t: (A.istft_adjoint_gpu(t, wa, wa1, 64, n_hops, 4),)
    check_layouts(fi, lays, fi(plain(g1)), what='istft_adjoint_gpu')
    n_hops = (301 - 1) // 16 + 1
    wa, wa1 = _win_powers(S, 'hann', None, 128, 1, dtype)
    assert A.istft_algo(dtype, 128, n_hops, 16, 301) == ('fused' if dtype == 'float32' else 'rocfft')
    fi = lambda t: (A.istft_adjoint_gpu(t, wa, wa1, 128, n_hops, 16),)
    check_layouts(fi, lays, fi(plain(g1)), what='istft_adjoint_gpu 128')
    K = 2
    cc, cw = _curves(301, K, 19, rng)
    upper, lower = np.clip(cc + cw, 0, 19), np.clip(cc - cw, 0, 19)
    upper[cc == -1], lower[cc == -1] = 0, 1
    lo, hi = lower.T, np.minimum(upper, 18).T
    gb = rng.standard_normal((2, K + 1, 301)).astype('float32').astype('float64')
    cdt = torch.complex64 if dtype == 'float32' else torch.complex128
    fb = lambda t: (A.band_colsum_adjoint(t, lo, hi, 19, cdt),)
    lays = [(nm, t.reshape(gb.shape)) for nm, t in real_layouts(gb.reshape(-1, 301))
            if nm in ('offset1', 'strided', 'fortran_batch', 'neg_bit', 'narrower_dtype')]
    check_layouts(fb, lays, fb(plain(gb)), what='band_colsum_adjoint')


def test_colsum_adjoint_output_pointer_alignment(S):
    """`ssq_colsum_adjoint` through the C ABI with the OUTPUT 8 bytes off a 16-byte boundary
    (complex64, even row length: the ``((uintptr_t)gZ & 15) == 0`` test of csrc/ssq_inverse.hip must
    send it to the 8-byte stores) and on one: the same values, and nothing written outside the array."""
    import torch
    from ssqueezepy_amd import _lib
    from ssqueezepy_amd._lib import check, F32
    lib = _lib.load()
    B, na, n = 2, 11, 300
    g = plain(_sig(n, B, 'float32'))
    size = B * na * n
    res = []
    for off in (0, 1):
        buf = torch.full((size + 2,), 7 + 7j, dtype=torch.complex64, device=DEV)
        out = buf[off:off + size]
        assert out.data_ptr() % 16 == 8 * off
        check(lib.ssq_colsum_adjoint(F32, g.data_ptr(), None, out.data_ptr(), B, na, n, S.algos.stream()))
        b = _np(buf)
        assert (b[:off] == 7 + 7j).all() and (b[off + size:] == 7 + 7j).all()
        res.append(b[off:off + size].reshape(B, na, n))
    assert np.array_equal(res[0], res[1])
    assert np.array_equal(res[1].real, np.repeat(_np(g)[:, None, :], na, axis=1)) and not res[1].imag.any()


def _offset_out(shape, dtype):
    """A dense array of `shape` one element into a buffer filled with a sentinel, one element to spare
    on either side: (buffer, view)."""
    import torch
    size = int(np.prod(shape))
    buf = torch.full((size + 2,), 7., dtype=dtype, device=DEV)
    view = buf[1:1 + size].view(shape)
    assert view.data_ptr() % 16 != 0
    return buf, view


@pytest.mark.parametrize('N', [2500, 2501])
def test_plan_outputs_at_element_aligned_pointers(S, N):
    """`ssq_cwt_execute` (column-tile path: the 16-byte `Wx` / `Tx` stores declared 8-byte aligned,
    csrc/ssq_tile_pair.hip `ssq_f4u`) and `ssq_stft_execute` (fused) through the C ABI with the signal
    AND every output one element past a 16-byte boundary -- include/ssq_hip.h asks for no more than
    an element's alignment: the bits of the call on torch's 256-byte aligned arrays, and the
    elements on either side of each output untouched. An even `N` keeps every row of the outputs 8
    bytes off; an odd one alternates."""
    import torch
    from ssqueezepy_amd import _cwt, _stft
    from ssqueezepy_amd._lib import check
    A = S.algos
    B = 2
    xb = _sig(N, B, 'float32', seed=5)
    xo = real_layouts(xb, only=('offset1',))[0][1]
    _cwt.clear_plan_cache()
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    Tx0, Wx0, _, _, dWx0 = S.ssq_cwt(plain(xb), wav, scales='log', nv=16, get_dWx=True)
    plan = list(_cwt._PLAN_CACHE.values())[-1]
    if os.environ.get('SSQ_CWT_TILES', '1') != '0':
        assert plan.tile_rows > 0.5 * plan.na
    outs = [_offset_out(Wx0.shape, torch.complex64) for _ in range(3)]
    check(plan.lib.ssq_cwt_execute(plan._h, xo.data_ptr(), B, outs[0][1].data_ptr(), outs[1][1].data_ptr(),
                                   outs[2][1].data_ptr(), None, 0, A.stream()))
    assert np.array_equal(_np(outs[0][1]), _np(Wx0)) and np.array_equal(_np(outs[1][1]), _np(dWx0))
    assert_tx_repeat(_np(outs[2][1]), _np(Tx0))
    for buf, _ in outs:
        assert complex(buf[0]) == 7 and complex(buf[-1]) == 7
    _cwt.clear_plan_cache()

    _stft._PLAN_CACHE.clear()
    Ts0, Sx0, _, _, dSx0 = S.ssq_stft(plain(xb), n_fft=128, hop_len=32, get_dWx=True)
    plan = _last_stft_plan()
    assert plan.algo == 'fused'
    outs = [_offset_out(Sx0.shape, torch.complex64) for _ in range(3)]
    check(plan.lib.ssq_stft_execute(plan._h, xo.data_ptr(), B, outs[0][1].data_ptr(), outs[1][1].data_ptr(),
                                    outs[2][1].data_ptr(), None, A.stream()))
    for (buf, got), want in zip(outs, (Sx0, dSx0, Ts0)):
        assert np.array_equal(_np(got), _np(want))
        assert complex(buf[0]) == 7 and complex(buf[-1]) == 7
    _stft._PLAN_CACHE.clear()


@pytest.mark.parametrize('dtype', DTYPES)
def test_input_side_gradient_layouts(S, dtype):
    """`x` a strided, an offset and (float32) a float64 non-leaf view of a leaf that requires grad: the
    gradient arrives at the leaf in the leaf's dtype and shape and equals the torch statement's
    (test_gpu_autograd.py's bound for an adjoint on a forward, 20 x 1e-5 / 1e-12). A conj view into
    `istft` / `issq_cwt` / `issq_stft`: the gradient `torch.autograd.grad` gives through
    `resolve_conj()`, bit for bit."""
    import torch
    tdt = torch.float32 if dtype == 'float32' else torch.float64
    N, n_fft, hop = 500, 128 if dtype == 'float32' else 100, 8
    rng = np.random.default_rng(9)
    xv = _sig(N, 0, dtype, seed=4)
    n_hops = (N - 1) // hop + 1
    wgt, wgt2 = _w((n_fft // 2 + 1, n_hops), 1), _w((n_fft // 2 + 1, n_hops), 2)
    views = {'strided': (2 * N, lambda l: l[::2], lambda g: g[::2]),
             'offset': (N + 1, lambda l: l[1:], lambda g: g[1:]),
             'float64_view': (N, lambda l: l.to(torch.float64), lambda g: g)}
    if dtype == 'float64':
        # (a float32 view of a float64 leaf carries a float32 gradient: torch rounds it before it reaches the leaf)
        del views['float64_view']
    for name, (size, view, pick) in views.items():
        leaf = torch.zeros(size, dtype=tdt, device=DEV)
        with torch.no_grad():
            (leaf if name == 'float64_view' else view(leaf)).copy_(torch.as_tensor(xv).to(DEV))
        leaf.requires_grad_(True)
        x = view(leaf)
        assert not x.is_leaf
        Sx, dSx = S.stft(x, n_fft=n_fft, hop_len=hop, derivative=True, dtype=dtype)
        _stft_loss(Sx, dSx, wgt.to(tdt), wgt2.to(tdt)).backward()
        assert leaf.grad.dtype == tdt and leaf.grad.shape == leaf.shape, name
        xr = torch.as_tensor(xv.astype(np.float64)).to(DEV).requires_grad_(True)
        Sr, dSr = torch_stft(S, xr, n_fft, hop, None, 'reflect', True, 1., dtype)
        _stft_loss(Sr, dSr, wgt, wgt2).backward()
        got = _np(leaf.grad).astype(np.float64)
        err = relmax(pick(got), _np(xr.grad))
        print("measured: input-side gradient", dtype, name, err)
        assert err <= 20 * TOL[dtype], (name, err)
        rest = got.copy()
        pick(rest)[...] = 0
        assert not rest.any(), name                          # the samples the view skips get no gradient

    cx = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(_cplx(dtype))
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    N2 = 677
    for what, v, f in (('istft', cx(n_fft // 2 + 1, (N2 - 1) // 16 + 1),
                        lambda t: S.istft(t, 'hann', n_fft=n_fft, hop_len=16, N=N2)),
                       ('issq_cwt', cx(33, 300), lambda t: S.issq_cwt(t, wav)),
                       ('issq_stft', cx(33, 300), lambda t: S.issq_stft(t, n_fft=64))):
        grads = []
        for resolve in (False, True):
            Sg = plain(v).requires_grad_(True)
            t = Sg.conj()
            assert t.is_conj()
            out = f(t.resolve_conj() if resolve else t)
            (g,) = torch.autograd.grad((out ** 2 * _w(out.shape, 5).to(out.dtype)).sum(), Sg)
            grads.append(g)
        assert float(grads[1].abs().max()) > 0
        assert torch.equal(torch.view_as_real(grads[0].resolve_conj()), torch.view_as_real(grads[1].resolve_conj())), what
        # ... and the forward is that of the conjugated values
        with torch.no_grad():
            assert torch.equal(f(plain(v).conj()), f(plain(np.conj(v)))), what


def test_gradcheck_strided_inputs(S):
    """`torch.autograd.gradcheck` (float64) on `stft` and `istft` with a strided view as the input."""
    import torch
    rng = np.random.default_rng(10)
    leaf = torch.as_tensor(rng.standard_normal(400)).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: S.stft(v[::2], n_fft=32, hop_len=8, dtype='float64'), (leaf,))
    n_fft, hop, N = 16, 4, 100
    n_hops = (N - 1) // hop + 1
    Z = rng.standard_normal((n_fft // 2 + 1, 2 * n_hops)) + 1j * rng.standard_normal((n_fft // 2 + 1, 2 * n_hops))
    Zl = torch.as_tensor(Z).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: S.istft(v[:, ::2], 'hann', n_fft=n_fft, hop_len=hop, N=N), (Zl,))
