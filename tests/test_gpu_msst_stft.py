# -*- coding: utf-8 -*-
"""`msst_stft`, `algos.multi_squeeze_gpu` and the entry `ssq_multi_squeeze` (the multisynchrosqueezing transform in one
kernel).

The oracle of the iteration is `msst.statement`: the entry's definition in NumPy on float64 arrays, one ufunc per
operation. The definition has only basic IEEE operations and the kernel evaluates the same operations in float64 in
the same order, so `wf` is compared with `==` in both dtypes. The expected `Tx` is `indexed_sum_onfly` on the
statement's `w_final`: the entry that is pinned to the oracle states the binning and the ordered accumulation, and
`Tx` is compared with `torch.equal`.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import msst
from msst import _np

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
ROWS = [2, 15, 16, 17, 33, 129]
COLS = [1, 3, 4, 5, 15, 16, 17, 33, 70]
N_ITERS = [1, 2, 3, 10]
# the row counts at which the launcher changes tile width -- the most rows of a 16-column and of an 8-column tile
# (msst.tile_rows: 160 KiB / (cols * 3 reals)) -- with the row after each, and the most rows of all
TILE_EDGES = ['rows16', 'rows16_plus_1', 'rows8', 'rows8_plus_1', 'max_rows']
N = 1024                # end to end


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def edge_rows(name, dtype):
    cols, plus = {'rows16': (16, 0), 'rows16_plus_1': (16, 1), 'rows8': (8, 0), 'rows8_plus_1': (8, 1),
                  'max_rows': (4, 0)}[name]
    return msst.tile_rows(dtype, cols) + plus


def max_rows(dtype):
    from ssqueezepy_amd import _lib
    return _lib.load().ssq_multi_squeeze_max_rows(_lib.F32 if dtype == 'float32' else _lib.F64)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def check_against_statement(S, Sx, w, Sfs, n_iter, interp, tag, **kw):
    """`wf` equal to the statement, `Tx` equal to `indexed_sum_onfly` on the statement's `w_final`."""
    import torch
    f0, df = msst.row_grid(Sfs)
    want_w = msst.statement(w, f0, df, n_iter, interp == 'linear')
    ssq_freqs = kw.pop('ssq_freqs', Sfs)
    const = kw.pop('const', 1)
    flipud = kw.pop('flipud', False)
    Tx, wf = S.multi_squeeze_gpu(Sx, w, Sfs, ssq_freqs, const, n_iter, interp, flipud, get_w=True)
    assert wf.dtype == dev(w).dtype and Tx.dtype == dev(Sx).dtype
    got_w = _np(wf)
    bad = got_w != want_w
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    want = S.indexed_sum_onfly(Sx, want_w, ssq_freqs, const, False, flipud)
    assert torch.equal(Tx, want), (tag, int((Tx != want).sum()))
    return Tx, want_w


# ------------------------------------------------------------------------------------------ kernel against statement
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', ROWS)
def test_kernel_vs_statement(S, rows, dtype, cols=COLS):
    moved = 0
    for n in cols:
        Sx, w, Sfs = msst.planes(1, rows, n, dtype)
        for interp in ('nearest', 'linear'):
            first = None
            for n_iter in N_ITERS:
                _, wf = check_against_statement(S, Sx, w, Sfs, n_iter, interp, (rows, n, dtype, interp, n_iter))
                first = wf if first is None else first
                moved += int((wf != first).sum())
    assert moved > 0                                     # the iteration did something


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('edge', TILE_EDGES)
def test_tile_width_edges(S, edge, dtype):
    """Both sides of every row count at which the launcher takes a narrower tile, and the most rows of all, n = 5."""
    rows = edge_rows(edge, dtype)
    if edge == 'max_rows':
        assert rows == max_rows(dtype) >= 1025
    Sx, w, Sfs = msst.planes(1, rows, 5, dtype)
    for interp, n_iter in (('linear', 3), ('nearest', 2)):
        check_against_statement(S, Sx, w, Sfs, n_iter, interp, (edge, dtype, interp))


# ------------------------------------------------------------------------------------------ crafted columns
ROWS_C, F0, DF = 24, 2., .5          # a grid whose arithmetic is exact


def run_column(S, wcol, dtype, n_iter, interp):
    """One column of `wcol` over ROWS_C rows: (wf, bins of the rows with a finite w), `Tx` checked on the way."""
    Sfs = (F0 + DF * np.arange(ROWS_C)).astype(dtype)
    rng = np.random.default_rng(1)
    Sx = (rng.standard_normal((1, ROWS_C, 1)) + 1j * rng.standard_normal((1, ROWS_C, 1))).astype(
        np.complex64 if dtype == 'float32' else np.complex128)
    w = np.asarray(wcol, dtype=dtype).reshape(1, ROWS_C, 1)
    check_against_statement(S, Sx, w, Sfs, n_iter, interp, ('column', dtype, n_iter, interp))
    return _np(S.multi_squeeze_gpu(Sx, w, Sfs, Sfs, 1, n_iter, interp, get_w=True)[1]).reshape(-1).astype(np.float64)


def at(k):
    return F0 + DF * np.asarray(k, dtype=np.float64)


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_crafted_columns(S, dtype, interp):
    i = np.arange(ROWS_C)
    inf = np.inf
    # w[i] = Sfs[i + 1]: n_iter = m lands every point on row min(i + m, rows - 1) (its frequency: row min(i + m, rows))
    for m in (1, 2, 5, ROWS_C + 3):
        assert np.array_equal(run_column(S, at(i + 1), dtype, m, interp), at(np.minimum(i + m, ROWS_C)))
    # a two-cycle between rows 3 and 9: the parity of n_iter decides
    w = np.full(ROWS_C, inf)
    w[3], w[9] = at(9), at(3)
    for m in (1, 2, 3, 10, 11):
        wf = run_column(S, w, dtype, m, interp)
        assert (wf[3], wf[9]) == ((at(9), at(3)) if m % 2 else (at(3), at(9))), m
        assert np.isinf(np.delete(wf, [3, 9])).all()
    # fixed points, reached in two passes at the most: n_iter = 1024 is n_iter = 3
    w = at(np.where(i % 3 == 0, i, np.where(i % 3 == 1, i - 1, i - 1)))
    a, b = run_column(S, w, dtype, 3, interp), run_column(S, w, dtype, 1024, interp)
    assert np.array_equal(a, b) and np.array_equal(a, at(i - i % 3))
    # a chain into an inf row stops in front of it: 0 -> 1 -> 2 -> 3 -> (4 holds nothing)
    w = np.full(ROWS_C, inf)
    w[:4] = at([1, 2, 3, 4])
    assert np.array_equal(run_column(S, w, dtype, 10, interp)[:4], at([4, 4, 4, 4]))
    # a chain that leaves the grid stops there; the final bin is clipped as ssq_indexed_sum clips (checked in Tx)
    w = np.full(ROWS_C, inf)
    w[:3] = at([1, 2, ROWS_C + 6.25])
    w[5], w[6] = at(6), at(-3.5)
    wf = run_column(S, w, dtype, 10, interp)
    assert np.array_equal(wf[:3], at([ROWS_C + 6.25] * 3)) and np.array_equal(wf[5:7], at([-3.5, -3.5]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_half_positions_and_missing_neighbours(S, dtype):
    inf = np.inf
    # nearest: positions exactly on .5 go half to even -- 2.5 -> row 2, 3.5 -> row 4
    w = np.full(ROWS_C, inf)
    w[0], w[1], w[2], w[4] = at(2.5), at(3.5), at(20), at(21)
    wf = run_column(S, w, dtype, 2, 'nearest')
    assert (wf[0], wf[1]) == (at(20), at(21))
    # linear: both neighbours finite -> interpolated; one inf -> the nearest row; the nearest row inf -> stays
    w = np.full(ROWS_C, inf)
    w[0], w[1], w[2] = at(10.25), at(12.25), at(12.75)
    w[10], w[11], w[12] = at(4), at(8), at(16)
    wf = run_column(S, w, dtype, 2, 'linear')
    assert wf[0] == at(4) + .25 * (at(8) - at(4))                # between rows 10 and 11
    assert wf[1] == at(16)                                       # row 13 holds nothing: the nearest row, 12
    assert wf[2] == at(12.75)                                    # the nearest row, 13, holds nothing: stop


# ------------------------------------------------------------------------------------------ link to indexed_sum_onfly
@pytest.mark.parametrize('flipud', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_one_pass_is_indexed_sum(S, dtype, flipud):
    import torch
    B, rows, n = 2, 33, 37
    Sx, w, Sfs = msst.planes(B, rows, n, dtype)
    other = np.linspace(5., 80., rows).astype(dtype)             # a grid of bins that is not the rows'
    rng = np.random.default_rng(2)
    consts = [1, 2.5, rng.uniform(.5, 2., rows).astype(np.float32), rng.uniform(.5, 2., rows)]
    for grid in (Sfs, other):
        for const in consts:
            Tx = S.multi_squeeze_gpu(Sx, w, Sfs, grid, const, 1, 'linear', flipud)
            assert torch.equal(Tx, S.indexed_sum_onfly(Sx, w, grid, const, False, flipud))
            # ... and with iterations the bins are taken on `grid`, the iteration on `Sfs`
            check_against_statement(S, Sx, w, Sfs, 4, 'linear', ('link', dtype, flipud), ssq_freqs=grid, const=const,
                                    flipud=flipud)


# ------------------------------------------------------------------------------------------ order
@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['one_bin', 'two_bins'])
def test_order(S, name, dtype, interp):
    """All rows of a column converge on one bin, or on two alternating ones, with cancelling pairs of terms up to 2^45
    among terms of order 1: another order of the additions gives other bits (tests/test_msst_design.py asserts that)."""
    Sx, w, Sfs, n_iter, final = msst.order_planes(dtype)[name]
    _, wf = check_against_statement(S, Sx, w, Sfs, n_iter, interp, (name, dtype, interp))
    assert np.array_equal(wf[0, :, 0].astype(np.float64), Sfs[final].astype(np.float64))


# ------------------------------------------------------------------------------------------ batch, repeat, layouts
@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    import torch
    Sx, w, Sfs = msst.planes(3, 33, 37, dtype)
    Sd, wd = dev(Sx), dev(w)
    Tx, wf = S.multi_squeeze_gpu(Sd, wd, Sfs, Sfs, 1, 5, 'linear', get_w=True)
    again = S.multi_squeeze_gpu(Sd, wd, Sfs, Sfs, 1, 5, 'linear', get_w=True)
    assert torch.equal(Tx, again[0]) and torch.equal(wf, again[1])
    for b in range(3):
        one = S.multi_squeeze_gpu(Sd[b], wd[b], Sfs, Sfs, 1, 5, 'linear', get_w=True)
        assert one[0].shape == Tx.shape[1:] and torch.equal(one[0], Tx[b]) and torch.equal(one[1], wf[b]), b


@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """Planes handed over as views -- a column slice (strided), a lazy conjugate, a pointer offset by one element,
    NumPy arrays -- and `out=` give the bits of the plain planes."""
    import torch
    B, rows, n = 2, 17, 21
    Sx, w, Sfs = msst.planes(B, rows, n, dtype)
    Sd, wd = dev(Sx), dev(w)

    def run(a, b, **kw):
        return S.multi_squeeze_gpu(a, b, Sfs, Sfs, 1, 4, 'linear', **kw)
    want = run(Sd, wd)
    big = torch.zeros((B, rows, n + 3), dtype=Sd.dtype, device=DEV)
    big[..., 1:-2] = Sd
    wbig = torch.zeros((B, rows, 2 * n), dtype=wd.dtype, device=DEV)
    wbig[..., ::2] = wd
    assert not big[..., 1:-2].is_contiguous() and not wbig[..., ::2].is_contiguous()
    assert torch.equal(run(big[..., 1:-2], wbig[..., ::2]), want)
    conj = dev(np.conj(Sx)).conj()
    assert conj.is_conj() and torch.equal(run(conj, wd), want)
    flat = torch.zeros(Sd.numel() + 1, dtype=Sd.dtype, device=DEV)
    flat[1:] = Sd.reshape(-1)
    wflat = torch.zeros(wd.numel() + 1, dtype=wd.dtype, device=DEV)
    wflat[1:] = wd.reshape(-1)
    shifted, wshifted = flat[1:].view(Sd.shape), wflat[1:].view(wd.shape)
    assert shifted.data_ptr() == flat.data_ptr() + Sd.element_size()
    assert torch.equal(run(shifted, wshifted), want)
    assert torch.equal(run(Sx, w), want)                          # NumPy planes
    assert torch.equal(run(Sd, w.astype(np.float64)), want)       # `w` of another dtype is cast to the planes'
    out = torch.full_like(Sd, -7.)
    assert run(Sd, wd, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError, match='`out`'):
        run(Sd, wd, out=out[..., ::2])
    with pytest.raises(ValueError, match='linearly'):
        S.multi_squeeze_gpu(Sd, wd, np.geomspace(1., 9., rows), Sfs)
    with pytest.raises(ValueError, match='linearly'):
        S.multi_squeeze_gpu(Sd, wd, Sfs, np.geomspace(1., 9., rows))
    with pytest.raises(ValueError, match='interp'):
        S.multi_squeeze_gpu(Sd, wd, Sfs, Sfs, interp='cubic')


# ------------------------------------------------------------------------------------------ refusals
def test_abi_refusals_leave_outputs_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert lib.ssq_version() >= 114 and _lib.ABI_VERSION >= 114 and 'ssq_multi_squeeze' in _lib.EXPORTS
    assert lib.ssq_multi_squeeze_max_rows(7) == 0
    B, rows, n = 1, 5, 11
    Sx, w, Sfs = msst.planes(B, rows, n, 'float64')
    Sd, wd, cst = dev(Sx), dev(w), dev(np.ones(rows))
    Tx = torch.full((B, rows, n), -7., dtype=torch.complex128, device=DEV)
    wf = torch.full((B, rows, n), -7., dtype=torch.float64, device=DEV)
    f0, df = msst.row_grid(Sfs)
    p = _lib.params5([f0, df])
    good = dict(Sx=Sd.data_ptr(), w=wd.data_ptr(), Tx=Tx.data_ptr(), wf=wf.data_ptr(), cst=cst.data_ptr(), batch=B,
                rows=rows, n=n, f0=f0, df=df, n_iter=3, interp=1, grid=_lib.GRID_LIN, params=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ssq_multi_squeeze(_lib.F64, a['Sx'], a['w'], a['Tx'], a['wf'], a['cst'], 0, a['batch'], a['rows'],
                                     a['n'], a['f0'], a['df'], a['n_iter'], a['interp'], a['grid'], a['params'], 0, None)
    nan, inf = float('nan'), float('inf')
    refused = [dict(Sx=None), dict(w=None), dict(Tx=None), dict(cst=None), dict(params=None), dict(batch=0),
               dict(n=0), dict(rows=1), dict(rows=0), dict(rows=max_rows('float64') + 1),
               dict(batch=1 << 20, rows=64, n=64), dict(n_iter=0), dict(n_iter=1025), dict(interp=2), dict(interp=-1),
               dict(df=0.), dict(df=-1.), dict(df=inf), dict(df=nan), dict(f0=inf), dict(f0=nan), dict(grid=3),
               dict(grid=-1)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_multi_squeeze'), (kw, lib.ssq_last_error())
        assert bool((Tx == -7.).all()) and bool((wf == -7.).all()), kw
    assert call(wf=None) == 0
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((Tx == -7.).any()) and bool((wf == -7.).all())
    assert call(n_iter=1024) == 0
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((wf == -7.).any())


# ------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize('dtype', DTYPES)
def test_column_sums_are_kept(S, dtype):
    """The transform moves terms along a column and loses none: ``Tx.sum(rows)`` against the n_iter = 1 result's, within
    ``2 rows eps(dtype) sum|terms|`` per column -- two orderings of the same terms."""
    B, rows, n = 2, 129, 33
    Sx, w, Sfs = msst.planes(B, rows, n, dtype)
    const = 1.5
    one = _np(S.multi_squeeze_gpu(Sx, w, Sfs, Sfs, const, 1)).astype(np.complex128).sum(axis=1)
    ten = _np(S.multi_squeeze_gpu(Sx, w, Sfs, Sfs, const, 10)).astype(np.complex128).sum(axis=1)
    terms = np.where(np.isfinite(w), np.abs(Sx).astype(np.float64) * const, 0.).sum(axis=1)
    bound = 2 * rows * msst.EPS[dtype] * terms
    report_measured('msst_column_sums_%s' % dtype, max_err_over_bound=float((np.abs(ten - one) / bound).max()))
    assert (np.abs(one) > 0).all() and (np.abs(ten - one) <= bound).all()


# ------------------------------------------------------------------------------------------ end to end
def stft_kw(dtype, hop=1):
    return dict(window=msst.gauss_window(), n_fft=msst.N_FFT, hop_len=hop, fs=msst.FS, dtype=dtype)


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_msst_stft_is_its_parts(S, dtype, order, N=N):
    import torch
    x = np.stack([msst.signal('linear', N)[0], msst.signal('fm', N)[0]])
    kw = stft_kw(dtype)
    Tx, Sx, ssq_freqs, Sfs, wf = S.msst_stft(x, n_iter=4, order=order, get_w=True, **kw)
    rows = msst.N_FFT // 2 + 1
    assert Tx.shape == Sx.shape == wf.shape == (2, rows, N) and Tx.grad_fn is None and not Tx.requires_grad
    assert np.array_equal(ssq_freqs, Sfs) and np.array_equal(Sfs, np.linspace(0, .5 * msst.FS, rows, dtype=dtype))
    # (`stft` with the derivative, the execution `ssq_stft` makes too: without it the plan takes another route to `Sx`)
    out = S.stft(x, derivative=True, **kw)
    assert torch.equal(Sx, out[0]) and torch.equal(Sx, S.ssq_stft(x, **kw)[1])
    gamma = 10 * msst.EPS[dtype]
    if order == 1:
        w = S.phase_stft(out[0], out[1], Sfs, gamma)
    else:
        w = S.ssq_stft2(x, get_w=True, **kw)[4]
    const = ssq_freqs[1] - ssq_freqs[0]
    want = S.multi_squeeze_gpu(Sx, w, Sfs, ssq_freqs, const, 4, 'linear', get_w=True)
    assert torch.equal(Tx, want[0]) and torch.equal(wf, want[1])
    for b in range(2):
        one = S.msst_stft(x[b], n_iter=4, order=order, **kw)
        assert len(one) == 4 and torch.equal(one[0], Tx[b]) and torch.equal(one[1], Sx[b])
    xt = torch.as_tensor(x[0]).to(DEV).requires_grad_(True)
    Tg = S.msst_stft(xt, n_iter=4, order=order, **kw)[0]
    assert Tg.grad_fn is None and torch.equal(Tg, Tx[0])
    outs = S.msst_stft(x[0], n_iter=4, order=order, astensor=False, get_w=True, flipud=True, **kw)
    assert all(isinstance(a, np.ndarray) for a in outs)
    assert np.array_equal(outs[0], _np(Tx[0])[::-1]) and np.array_equal(outs[2], Sfs[::-1])
    assert np.array_equal(outs[4], _np(wf[0]))
    if order == 1:
        # one pass is the first-order transform: ssq_stft2 with chirp_tol = inf, indexed_sum_onfly on phase_stft's w
        assert torch.equal(S.msst_stft(x, n_iter=1, **kw)[0], S.ssq_stft2(x, chirp_tol=np.inf, **kw)[0])
    with pytest.raises(ValueError, match='order'):
        S.msst_stft(x[0], order=3, **kw)


@pytest.mark.parametrize('dtype', DTYPES)
def test_inverse(S, dtype, N=N):
    """`issq_stft` on `msst_stft`'s `Tx` at n_iter = 10 reconstructs the signal no worse than on `ssq_stft`'s for the
    same call, times 1.05 (the margin: another grouping of the same sums)."""
    x = msst.signal('linear', N)[0] + .5 * msst.signal('fm', N)[0]
    kw = dict(stft_kw(dtype), fs=1.)             # (`issq_stft` takes `Tx` as made with the frequencies in cycles per sample)
    errs = {}
    for name, Tx in (('ssq_stft', S.ssq_stft(x, **kw)[0]), ('msst_stft', S.msst_stft(x, n_iter=10, **kw)[0])):
        xr = _np(S.issq_stft(Tx, window=kw['window'], n_fft=msst.N_FFT)).astype(np.float64)
        errs[name] = float(np.abs(xr - x).mean() / np.abs(x).mean())
    report_measured('msst_inverse_%s_N%d' % (dtype, N), **errs)
    assert errs['ssq_stft'] < 1e-2                        # the reference point reconstructs the signal at all
    assert errs['msst_stft'] <= 1.05 * errs['ssq_stft'], errs


# ------------------------------------------------------------------------------------------ what the transform buys
def shares(S, name, dtype, passes, N=N):
    x, f = msst.signal(name, N)
    out = {}
    for n_iter, interp in passes:
        Tx, _, ssq_freqs, _ = S.msst_stft(x, n_iter=n_iter, interp=interp, **stft_kw(dtype))
        out[(n_iter, interp)] = msst.share(Tx, f, ssq_freqs)
    return out


@pytest.mark.parametrize('dtype', DTYPES)
def test_linear_chirp_is_sharpened(S, dtype, N=N):
    """The linear chirp 50 -> 450 Hz: the share of ``|Tx|^2`` within +-1 bin of the true frequency at n_iter = 10,
    linear, is >= 0.95, exceeds the n_iter = 1 share by >= 0.3 and the nearest-row form's by >= 0.2. (A float64
    prototype with an analytic derivative window gave 0.998, 0.404 and 0.450.)"""
    s = shares(S, 'linear', dtype, [(1, 'linear'), (10, 'linear'), (10, 'nearest')], N)
    report_measured('msst_linear_chirp_%s_N%d' % (dtype, N), one=s[(1, 'linear')], ten=s[(10, 'linear')],
                    ten_nearest=s[(10, 'nearest')])
    assert s[(10, 'linear')] >= .95
    assert s[(10, 'linear')] - s[(1, 'linear')] >= .3
    assert s[(10, 'linear')] - s[(10, 'nearest')] >= .2


@pytest.mark.parametrize('dtype', DTYPES)
def test_fm_tone_is_sharpened(S, dtype, N=N):
    """The FM tone 150 +- 60 Hz at 2 Hz: the share at n_iter = 20 exceeds the n_iter = 1 share by >= 0.1. (Prototype:
    0.935 against 0.631.)"""
    s = shares(S, 'fm', dtype, [(1, 'linear'), (20, 'linear')], N)
    report_measured('msst_fm_tone_%s_N%d' % (dtype, N), one=s[(1, 'linear')], twenty=s[(20, 'linear')])
    assert s[(20, 'linear')] - s[(1, 'linear')] >= .1
