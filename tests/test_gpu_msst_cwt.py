# -*- coding: utf-8 -*-
"""`msst_cwt`, `algos.multi_squeeze_cwt_gpu` and the entry `ssq_multi_squeeze_cwt` (the multisynchrosqueezing transform
on a table of rows in one kernel).

The oracle of the iteration is `msst_cwt.statement`: the entry's definition in NumPy on float64 arrays, one ufunc per
operation, the interval from `np.searchsorted`. The definition has only comparisons against the table and basic IEEE
operations, and the kernel evaluates the same operations in float64 in the same order, so `wf` is compared with `==`
in both dtypes. The expected `Tx` is `indexed_sum_onfly` on the statement's `w_final` and the same grid: the entry that
is pinned to the oracle states the binning and the ordered accumulation, and `Tx` is compared with `torch.equal`.
"""
import os
import numpy as np
import pytest
from conftest import report_measured
import msst
import msst_cwt as M
from msst import _np

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
N_ITERS = [1, 2, 10]
# (table, rows, n): the library's own tables have 33 and 245 rows
TABLE_CASES = [('log', 40, 21), ('log-piecewise', 33, 17), ('log-piecewise', 245, 9), ('hyperbolic', 40, 21),
               ('linear-ascending', 40, 21), ('irregular', 40, 21), ('irregular', 131, 7), ('jittered', 131, 7)]
SMALL_ROWS = [2, 3, 17, 31, 33]
N = 1024                # end to end


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def code(dtype):
    from ssqueezepy_amd import _lib
    return _lib.F32 if dtype == 'float32' else _lib.F64


def lib_tile(dtype, rows):
    from ssqueezepy_amd import _lib
    return _lib.load().ssq_multi_squeeze_cwt_tile(code(dtype), rows)


def max_rows(dtype):
    from ssqueezepy_amd import _lib
    return _lib.load().ssq_multi_squeeze_cwt_max_rows(code(dtype))


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def is_log(grid):
    from ssqueezepy_amd.scales import infer_scaletype
    grid = np.asarray(grid)
    return bool(len(grid) > 2 and infer_scaletype(grid)[0].startswith('log'))


def check_against_statement(S, Wx, w, fr, grid, n_iter, interp, tag, const=1, flipud=False):
    """`wf` equal to the statement, `Tx` equal to `indexed_sum_onfly` on the statement's `w_final`."""
    import torch
    want_w = M.statement(w, fr, n_iter, interp == 'linear')
    Tx, wf = S.multi_squeeze_cwt_gpu(Wx, w, fr, grid, const, n_iter, interp, flipud, get_w=True)
    assert wf.dtype == dev(w).dtype and Tx.dtype == dev(Wx).dtype
    got_w = _np(wf)
    bad = got_w != want_w
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    want = S.indexed_sum_onfly(Wx, want_w, grid, const, is_log(grid), flipud)
    assert torch.equal(Tx, want), (tag, int((Tx != want).sum()))
    return Tx, want_w


# ------------------------------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', TABLE_CASES, ids=lambda c: '%s_%d' % c[:2])
def test_tables(S, case, dtype):
    """Every kind of table, `w` uniform over 1.5 times its range with a quarter ``inf`` and three NaN; n_iter 1, 2, 10,
    both `interp`, both `flipud`, the bins on a grid of each kind."""
    kind, rows, n = case
    fr, metric = M.table(kind, rows)
    Wx, w = M.planes(1, rows, n, dtype, fr, metric)
    assert np.isnan(w).sum() == 3 and np.isinf(w).sum() > rows * n // 8
    moved = 0
    for gk in M.grids_for(rows):
        grid = M.bin_grid(gk, fr)
        for interp in ('nearest', 'linear'):
            first = None
            for n_iter in N_ITERS:
                for flipud in (False, True):
                    _, wf = check_against_statement(S, Wx, w, fr, grid, n_iter, interp,
                                                    (kind, rows, dtype, gk, interp, n_iter, flipud), flipud=flipud)
                first = wf if first is None else first
                with np.errstate(invalid='ignore'):
                    moved += int((wf != first).sum())
    assert moved > 0                                     # the iteration did something


# ------------------------------------------------------------------------------------------ 2. sizes
def edges(dtype):
    """The row counts on both sides of every edge `ssq_multi_squeeze_cwt_tile` reports, found from the query alone."""
    top = max_rows(dtype)
    out = []
    for rows in range(2, top + 1):
        if lib_tile(dtype, rows) != lib_tile(dtype, rows + 1):
            out += [rows, rows + 1]
    return out, top


@pytest.mark.parametrize('dtype', DTYPES)
def test_tile_edges_and_most_rows(S, dtype):
    """Both sides of every row count at which the launcher takes a narrower tile, and the most rows of all, n = 5;
    one row more than the most is refused."""
    from ssqueezepy_amd import _lib
    rows_at, top = edges(dtype)
    assert rows_at == [M.tile_rows(dtype, 16), M.tile_rows(dtype, 16) + 1, M.tile_rows(dtype, 8),
                       M.tile_rows(dtype, 8) + 1, top, top + 1] and top == M.tile_rows(dtype, 4)
    assert [lib_tile(dtype, r) for r in rows_at] == [16, 8, 8, 4, 4, 0]
    for rows in rows_at[:-1]:
        fr, metric = M.table('irregular', rows)
        Wx, w = M.planes(1, rows, 5, dtype, fr, metric)
        grid = M.bin_grid('log', fr)
        for interp, n_iter in (('linear', 3), ('nearest', 2)):
            check_against_statement(S, Wx, w, fr, grid, n_iter, interp, (rows, dtype, interp))
    rows = top + 1
    fr, metric = M.table('irregular', rows)
    Wx, w = M.planes(1, rows, 5, dtype, fr, metric)
    with pytest.raises(_lib.SsqError, match='ssq_multi_squeeze_cwt: %d rows, at most %d' % (rows, top)):
        S.multi_squeeze_cwt_gpu(Wx, w, fr, M.bin_grid('log', fr))


def tile_rows_for(dtype, cols):
    """The row count the column counts around a tile of `cols` columns run at. A tile's width follows from the rows
    alone, so the 8- and 4-column tiles are met at the first row count that takes them."""
    return {16: 19, 8: M.tile_rows(dtype, 16) + 1, 4: M.tile_rows(dtype, 8) + 1}[cols]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cols', [16, 8, 4])
def test_column_counts_around_the_tiles(S, cols, dtype):
    rows = tile_rows_for(dtype, cols)
    assert lib_tile(dtype, rows) == cols
    ns = {16: [1, 3, 4, 5, 15, 16, 17, 33], 8: [1, 7, 8, 9, 17], 4: [3, 4, 5, 9]}[cols]
    fr, metric = M.table('log', rows)
    grid = M.bin_grid('log', fr)
    for n in ns:
        Wx, w = M.planes(1, rows, n, dtype, fr, metric)
        check_against_statement(S, Wx, w, fr, grid, 3, 'linear', (cols, rows, n, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', SMALL_ROWS)
def test_row_counts_off_the_lanes(S, rows, dtype):
    """Rows that are no multiple of the 16 row-lanes or of the 32 rows of a step, down to the fewest."""
    for kind in ('irregular', 'linear-ascending'):
        fr, metric = M.table(kind, rows)
        for n in (5, 21):
            Wx, w = M.planes(1, rows, n, dtype, fr, metric)
            for gk in M.grids_for(rows):
                for interp in ('nearest', 'linear'):
                    check_against_statement(S, Wx, w, fr, M.bin_grid(gk, fr), 4, interp, (kind, rows, n, dtype, gk))


# ------------------------------------------------------------------------------------------ 3. crafted columns
def run_column(S, wcol, fr, dtype, n_iter, interp):
    """One column of `wcol` over the rows of `fr`: `wf` in float64, `Tx` checked on the way."""
    rows = len(fr)
    rng = np.random.default_rng(1)
    Wx = (rng.standard_normal((1, rows, 1)) + 1j * rng.standard_normal((1, rows, 1))).astype(
        np.complex64 if dtype == 'float32' else np.complex128)
    w = np.asarray(wcol, dtype=dtype).reshape(1, rows, 1)
    _, wf = check_against_statement(S, Wx, w, fr, M.bin_grid('linear', fr), n_iter, interp,
                                    ('column', dtype, n_iter, interp))
    return wf.reshape(-1).astype(np.float64)


@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_crafted_columns(S, dtype, interp):
    M.crafted_cases(lambda wcol, fr, m, ip: run_column(S, wcol, fr, dtype, m, ip), dtype, interp)


@pytest.mark.parametrize('dtype', DTYPES)
def test_half_positions_and_missing_neighbours(S, dtype):
    M.half_and_neighbour_cases(lambda wcol, fr, m, ip: run_column(S, wcol, fr, dtype, m, ip))


# ------------------------------------------------------------------------------------------ 4. link to the linear kernel
@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_link_to_the_linear_kernel(S, dtype, interp):
    """An ascending table ``2 + i / 2`` with every `w` a multiple of 1/8: both position rules are exact, so the two
    entries agree bit for bit; the table reversed with the rows reversed gives the row-reversed `wf`."""
    import torch
    B, rows, n = 2, 37, 19
    rng = np.random.default_rng(4)
    Sfs = 2. + .5 * np.arange(rows)
    cdt = np.complex64 if dtype == 'float32' else np.complex128
    Wx = (rng.standard_normal((B, rows, n)) + 1j * rng.standard_normal((B, rows, n))).astype(cdt)
    w = (rng.integers(0, 8 * (rows // 2 + 6), (B, rows, n)) / 8.).astype(dtype)       # 0 .. above the last row
    w[rng.uniform(size=w.shape) < .2] = np.inf
    for n_iter in (2, 3, 10):
        Tc, wc = S.multi_squeeze_cwt_gpu(Wx, w, Sfs, Sfs, 1, n_iter, interp, get_w=True)
        Tl, wl = S.multi_squeeze_gpu(Wx, w, Sfs, Sfs, 1, n_iter, interp, get_w=True)
        assert torch.equal(Tc, Tl) and torch.equal(wc, wl), n_iter
        assert np.array_equal(_np(wc), M.statement(w, Sfs, n_iter, interp == 'linear'))
        # (37 rows: a row keeps its parity under the reversal, so half to the even row picks the same row)
        wr = S.multi_squeeze_cwt_gpu(Wx[:, ::-1], w[:, ::-1], Sfs[::-1], Sfs, 1, n_iter, interp, get_w=True)[1]
        assert np.array_equal(_np(wr)[:, ::-1], _np(wc)), n_iter
    assert (_np(wc) != w).any()


# ------------------------------------------------------------------------------------------ 5. one pass
@pytest.mark.parametrize('flipud', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_one_pass_is_indexed_sum(S, dtype, flipud):
    import torch
    B, rows, n = 2, 33, 37
    fr, metric = M.table('log', rows)
    Wx, w = M.planes(B, rows, n, dtype, fr, metric)
    rng = np.random.default_rng(2)
    consts = [1, 2.5, rng.uniform(.5, 2., rows).astype(np.float32), rng.uniform(.5, 2., rows)]
    for gk in M.GRIDS:
        grid = M.bin_grid(gk, fr)
        for const in consts:
            Tx = S.multi_squeeze_cwt_gpu(Wx, w, fr, grid, const, 1, 'linear', flipud)
            # (a NaN in `w`: skipped here like an inf, put in a bin by indexed_sum_onfly -- compared on the finite-or-inf w)
            wi = np.where(np.isnan(w), np.inf, w)
            assert torch.equal(Tx, S.indexed_sum_onfly(Wx, wi, grid, const, gk != 'linear', flipud)), (gk, const)


# ------------------------------------------------------------------------------------------ 6. order
@pytest.mark.parametrize('interp', ['nearest', 'linear'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['one_bin', 'two_bins'])
def test_order(S, name, dtype, interp):
    """All rows of a column converge on one bin, or on two alternating ones, with cancelling pairs of terms up to 2^45
    among terms of order 1: `Tx` is the ascending-row sum and not the descending one."""
    Sx, w, fr, Sfs, n_iter, bins, f_final = M.order_case(name, dtype)
    Tx, wf = check_against_statement(S, Sx, w, fr, Sfs, n_iter, interp, (name, dtype, interp))
    assert np.array_equal(wf[0, :, 0].astype(np.float64), f_final)
    fwd, rev = msst.ordered_sum(Sx, bins, 1.), msst.ordered_sum(Sx, bins, 1., reverse=True)
    got = _np(Tx)
    assert np.array_equal(got, fwd) and (got != rev).any()


# ------------------------------------------------------------------------------------------ 7. batch, layouts, refusals
@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    import torch
    fr, metric = M.table('irregular', 33)
    Wx, w = M.planes(3, 33, 37, dtype, fr, metric)
    grid = M.bin_grid('log', fr)
    Wd, wd = dev(Wx), dev(w)
    Tx, wf = S.multi_squeeze_cwt_gpu(Wd, wd, fr, grid, 1, 5, 'linear', get_w=True)
    again = S.multi_squeeze_cwt_gpu(Wd, wd, fr, grid, 1, 5, 'linear', get_w=True)
    assert torch.equal(Tx, again[0]) and torch.equal(wf, again[1])
    for b in range(3):
        one = S.multi_squeeze_cwt_gpu(Wd[b], wd[b], fr, grid, 1, 5, 'linear', get_w=True)
        assert one[0].shape == Tx.shape[1:] and torch.equal(one[0], Tx[b]) and torch.equal(one[1], wf[b]), b


@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts_and_python_refusals(S, dtype):
    """Planes handed over as views -- a column slice (strided), a lazy conjugate, a pointer offset by one element,
    NumPy arrays --, a table given as a tensor or in another dtype, `out=` and `get_w` give the bits of the plain
    call; what the Python layer refuses."""
    import torch
    B, rows, n = 2, 17, 21
    fr, metric = M.table('log', rows)
    Wx, w = M.planes(B, rows, n, dtype, fr, metric)
    grid = M.bin_grid('log', fr)
    Wd, wd = dev(Wx), dev(w)

    def run(a, b, table=fr, **kw):
        return S.multi_squeeze_cwt_gpu(a, b, table, grid, 1, 4, 'linear', **kw)
    want, want_w = run(Wd, wd, get_w=True)
    assert isinstance(run(Wd, wd), torch.Tensor) and torch.equal(run(Wd, wd), want)
    big = torch.zeros((B, rows, n + 3), dtype=Wd.dtype, device=DEV)
    big[..., 1:-2] = Wd
    wbig = torch.zeros((B, rows, 2 * n), dtype=wd.dtype, device=DEV)
    wbig[..., ::2] = wd
    assert not big[..., 1:-2].is_contiguous() and not wbig[..., ::2].is_contiguous()
    assert torch.equal(run(big[..., 1:-2], wbig[..., ::2]), want)
    conj = dev(np.conj(Wx)).conj()
    assert conj.is_conj() and torch.equal(run(conj, wd), want)
    flat = torch.zeros(Wd.numel() + 1, dtype=Wd.dtype, device=DEV)
    flat[1:] = Wd.reshape(-1)
    wflat = torch.zeros(wd.numel() + 1, dtype=wd.dtype, device=DEV)
    wflat[1:] = wd.reshape(-1)
    shifted, wshifted = flat[1:].view(Wd.shape), wflat[1:].view(wd.shape)
    assert shifted.data_ptr() == flat.data_ptr() + Wd.element_size()
    assert torch.equal(run(shifted, wshifted), want)
    assert torch.equal(run(Wx, w), want)                          # NumPy planes
    assert torch.equal(run(Wd, w.astype(np.float64)), want)       # `w` of another dtype is cast to the planes'
    assert torch.equal(run(Wd, wd, table=dev(fr)), want)          # the table as a device tensor
    assert torch.equal(run(Wd, wd, table=np.asfortranarray(fr.reshape(1, -1))), want)
    out = torch.full_like(Wd, -7.)
    got = run(Wd, wd, out=out, get_w=True)
    assert got[0] is out and torch.equal(out, want) and torch.equal(got[1], want_w)
    with pytest.raises(ValueError, match='`out`'):
        run(Wd, wd, out=out[..., ::2])
    with pytest.raises(ValueError, match='one entry per row'):
        run(Wd, wd, table=fr[:-1])
    nan_table, twice, bent = fr.copy(), fr.copy(), fr.copy()
    nan_table[5] = np.nan
    twice[6] = twice[5]
    bent[6] = bent[4]
    with pytest.raises(ValueError, match='finite'):
        run(Wd, wd, table=nan_table)
    with pytest.raises(ValueError, match='strictly monotone'):
        run(Wd, wd, table=twice)
    with pytest.raises(ValueError, match='strictly monotone'):
        run(Wd, wd, table=bent)
    with pytest.raises(ValueError, match='one entry per row'):
        S.multi_squeeze_cwt_gpu(Wd, wd, fr, grid[:-1])
    with pytest.raises(ValueError, match='interp'):
        S.multi_squeeze_cwt_gpu(Wd, wd, fr, grid, interp='cubic')
    with pytest.raises(ValueError, match='shapes differ'):
        S.multi_squeeze_cwt_gpu(Wd, wd[..., :-1], fr, grid)


def test_abi_refusals_leave_outputs_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert lib.ssq_version() >= 119 and _lib.ABI_VERSION >= 119
    assert {'ssq_multi_squeeze_cwt', 'ssq_multi_squeeze_cwt_max_rows', 'ssq_multi_squeeze_cwt_tile'} <= set(_lib.EXPORTS)
    assert lib.ssq_multi_squeeze_cwt_max_rows(7) == 0 and lib.ssq_multi_squeeze_cwt_tile(7, 10) == 0
    assert lib.ssq_multi_squeeze_cwt_tile(_lib.F64, 1) == 0 and lib.ssq_multi_squeeze_cwt_tile(_lib.F64, 2) == 16
    B, rows, n = 1, 5, 11
    fr, metric = M.table('log', rows)
    Wx, w = M.planes(B, rows, n, 'float64', fr, metric)
    Wd, wd, cst = dev(Wx), dev(w), dev(np.ones(rows))
    Tx = torch.full((B, rows, n), -7., dtype=torch.complex128, device=DEV)
    wf = torch.full((B, rows, n), -7., dtype=torch.float64, device=DEV)
    grid = M.bin_grid('linear', fr)
    p = _lib.params5([grid[0], grid[1] - grid[0]])

    def table(v):
        return np.ascontiguousarray(v, dtype=np.float64)
    fr = table(fr)
    big = table(M.table('log', max_rows('float64') + 1)[0])
    good = dict(Wx=Wd.data_ptr(), w=wd.data_ptr(), Tx=Tx.data_ptr(), wf=wf.data_ptr(), cst=cst.data_ptr(), fr=fr,
                batch=B, rows=rows, n=n, n_iter=3, interp=1, grid=_lib.GRID_LIN, params=p)

    def call(**kw):
        a = dict(good, **kw)
        t = a['fr']
        return lib.ssq_multi_squeeze_cwt(_lib.F64, a['Wx'], a['w'], a['Tx'], a['wf'], a['cst'], 0,
                                         None if t is None else t.ctypes.data, a['batch'], a['rows'], a['n'],
                                         a['n_iter'], a['interp'], a['grid'], a['params'], 0, None)
    nan, inf = float('nan'), float('inf')

    def with_(i, v):
        t = fr.copy()
        t[i] = v
        return t
    refused = [dict(Wx=None), dict(w=None), dict(Tx=None), dict(cst=None), dict(fr=None), dict(params=None),
               dict(batch=0), dict(n=0), dict(rows=1), dict(rows=0), dict(rows=len(big), fr=big),
               dict(batch=1 << 20, rows=64, n=64, fr=table(M.table('log', 64)[0])), dict(n_iter=0), dict(n_iter=1025),
               dict(interp=2), dict(interp=-1), dict(fr=with_(2, nan)), dict(fr=with_(0, inf)), dict(fr=with_(4, -inf)),
               dict(fr=with_(1, nan)), dict(fr=with_(3, fr[2])), dict(fr=with_(3, fr[1])), dict(fr=with_(4, fr[0])),
               dict(fr=with_(1, fr[0])), dict(grid=3), dict(grid=-1)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_multi_squeeze_cwt'), (kw, lib.ssq_last_error())
        assert bool((Tx == -7.).all()) and bool((wf == -7.).all()), kw
    assert lib.ssq_multi_squeeze_cwt(7, *[None] * 5, 0, None, 1, 2, 1, 1, 0, 2, None, 0, None) != 0
    assert lib.ssq_last_error().decode().startswith('ssq_multi_squeeze_cwt')
    assert call(wf=None) == 0
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((Tx == -7.).any()) and bool((wf == -7.).all())
    assert call(n_iter=1024, fr=table(fr[::-1])) == 0             # (an ascending table is as good)
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((wf == -7.).any())


# ------------------------------------------------------------------------------------------ 8. column sums
@pytest.mark.parametrize('dtype', DTYPES)
def test_column_sums_are_kept(S, dtype):
    """The transform moves terms along a column and loses none: with a constant weight a column's sum is `const` times
    the sum of its rows with a finite `w` (a NaN is skipped), within ``2 rows eps(dtype) sum|terms|`` per column -- two
    orderings of the same terms."""
    B, rows, n = 2, 129, 33
    fr, metric = M.table('log', rows)
    Wx, w = M.planes(B, rows, n, dtype, fr, metric)
    grid = M.bin_grid('log', fr)
    const = 1.5
    fin = np.isfinite(w)
    assert np.isnan(w).any()
    direct = const * np.where(fin, Wx.astype(np.complex128), 0.).sum(axis=1)
    terms = np.where(fin, np.abs(Wx).astype(np.float64) * const, 0.).sum(axis=1)
    bound = 2 * rows * msst.EPS[dtype] * terms
    worst = 0.
    for n_iter in (1, 10):
        got = _np(S.multi_squeeze_cwt_gpu(Wx, w, fr, grid, const, n_iter)).astype(np.complex128).sum(axis=1)
        worst = max(worst, float((np.abs(got - direct) / bound).max()))
        assert (np.abs(got) > 0).all() and (np.abs(got - direct) <= bound).all(), n_iter
    report_measured('msst_cwt_column_sums_%s' % dtype, max_err_over_bound=worst)


# ------------------------------------------------------------------------------------------ 9. end to end
def x_pair(N):
    return np.stack([M.signal('chirp', N)[0], M.signal('fm', N)[0]])


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_msst_cwt_is_its_parts(S, dtype, order, N=N):
    import torch
    from ssqueezepy_amd import Wavelet
    from ssqueezepy_amd.wavelets import row_frequencies
    x = x_pair(N)
    wav = M.make_wavelet('gmw', N, dtype)
    kw = dict(wavelet=wav, nv=16)
    Tx, Wx, ssq_freqs, scales, wf = S.msst_cwt(x, n_iter=4, order=order, get_w=True, **kw)
    rows = len(scales)
    assert Tx.shape == Wx.shape == wf.shape == (2, rows, N) and Tx.grad_fn is None and not Tx.requires_grad
    assert Tx.dtype == Wx.dtype == (torch.complex64 if dtype == 'float32' else torch.complex128)
    # the parts: ssq_cwt's plan execution, the map, the kernel
    ref = S.ssq_cwt(x, get_dWx=True, **kw)
    assert torch.equal(Wx, ref[1]) and np.array_equal(ssq_freqs, ref[2]) and np.array_equal(scales, ref[3])
    gamma = 10 * msst.EPS[dtype]
    if order == 1:
        w = S.phase_cwt(Wx, ref[4], gamma=gamma)
    else:
        w = S.ssq_cwt2(x, get_w=True, **kw)[4]
    fr = row_frequencies(wav, scales)
    assert (np.diff(fr) < 0).all() and np.array_equal(fr, row_frequencies(wav, scales, fs=1.))
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    const = _ssq_design(wav, 'log-piecewise', 16, N, 1., None, 'peak', True)[2]
    want = S.multi_squeeze_cwt_gpu(Wx, w, fr, ssq_freqs[::-1], const, 4, 'linear', True, get_w=True)
    assert torch.equal(Tx, want[0]) and torch.equal(wf, want[1])
    for b in range(2):
        one = S.msst_cwt(x[b], n_iter=4, order=order, **kw)
        assert len(one) == 4 and torch.equal(one[0], Tx[b]) and torch.equal(one[1], Wx[b])
    xt = torch.as_tensor(x[0]).to(DEV).requires_grad_(True)
    Tg = S.msst_cwt(xt, n_iter=4, order=order, **kw)[0]
    assert Tg.grad_fn is None and torch.equal(Tg, Tx[0])
    outs = S.msst_cwt(x[0], n_iter=4, order=order, astensor=False, get_w=True, flipud=False, **kw)
    assert all(isinstance(a, np.ndarray) for a in outs)
    assert np.array_equal(outs[0], _np(Tx[0])[::-1]) and np.array_equal(outs[2], ssq_freqs)
    assert np.array_equal(outs[4], _np(wf[0]))
    # one pass is the first-order transform (the second-order one for order = 2) as indexed_sum_onfly computes it
    one_pass = S.msst_cwt(x, n_iter=1, order=order, **kw)[0]
    assert torch.equal(one_pass, S.indexed_sum_onfly(Wx, w, ssq_freqs[::-1], const, True, True))
    if order == 2:
        assert torch.equal(one_pass, S.ssq_cwt2(x, **kw)[0])
    with pytest.raises(ValueError, match='order'):
        S.msst_cwt(x[0], order=3, **kw)
    if order == 1:
        # any wavelet: one without closed-form companions
        bump = Wavelet('bump', N=N, dtype=dtype)
        assert S.msst_cwt(x[0], wavelet=bump, nv=8, n_iter=3)[0].shape[-1] == N
        with pytest.raises(Exception):
            S.msst_cwt(x[0], wavelet=bump, nv=8, n_iter=3, order=2)


# The error of `issq_cwt` on `msst_cwt`'s `Tx` over its error on `ssq_cwt`'s, same call. The inverse sums a column of
# `Tx`, and the transform only moves terms within a column, so the two differ by the rounding of two orders of one sum:
# measured ratio - 1 (profiles/msst_cwt.txt) 2.1e-6 in float32, below 1e-14 in float64, against an error of 1.3e-3.
INVERSE_MARGIN = 1.001


@pytest.mark.parametrize('dtype', DTYPES)
def test_inverse(S, dtype, N=N):
    """`issq_cwt` on `msst_cwt`'s `Tx` at n_iter = 10 reconstructs the signal: its error is that of `issq_cwt` on
    `ssq_cwt`'s `Tx` for the same call times at most `INVERSE_MARGIN` -- the transform moves terms within a column, and
    the inverse sums the column."""
    x = M.signal('chirp', N)[0] + .5 * M.signal('fm', N)[0]
    wav = M.make_wavelet('gmw', N, dtype)
    errs = {}
    for name, Tx in (('ssq_cwt', S.ssq_cwt(x, wav)[0]), ('msst_cwt', S.msst_cwt(x, wav, n_iter=10)[0])):
        xr = _np(S.issq_cwt(Tx, wav)).astype(np.float64)
        errs[name] = float(np.abs(xr - x).mean() / np.abs(x).mean())
    report_measured('msst_cwt_inverse_%s_N%d' % (dtype, N), **errs)
    assert errs['ssq_cwt'] < .2                           # the reference point reconstructs the signal at all
    assert errs['msst_cwt'] <= INVERSE_MARGIN * errs['ssq_cwt'], errs


# ------------------------------------------------------------------------------------------ 10. what the transform buys
# |share on the device - share of the NumPy float64 restatement|, at most. What differs is the bin of single points that
# lie on a rounding boundary of the bin map (the planes agree to the dtype's precision, `log2` to an ulp); a ridge
# point holds up to about 1e-4 of a signal's energy. Measured: 2.7e-5 at the most in float32
# (the Morlet FM tone), 2.3e-6 in float64 under the emulator's FFT and 3.1e-9 on the device. The smallest gap between two
# shares that the inequalities below compare is 0.0047.
SHARE_MARGIN = {'float32': 1e-4, 'float64': 1e-4}
# share(10 passes) >= share(5 passes) - SLACK. Measured: ten passes exceed five by 0.0047 (the chirp) to 0.022 on
# every signal, in both dtypes and in the restatement, so none is needed here; the dip of the issue's prototype
# belongs to a faster modulation, where the map stops being a contraction.
SLACK = 0.


def shares(S, name, dtype):
    kind, n, wavelet = M.SIGNALS[name]
    x, f = M.signal(kind, n)
    wav = M.make_wavelet(wavelet, n, dtype)
    out = {}
    for n_iter, interp in M.PASSES:
        Tx, _, ssq_freqs, _ = S.msst_cwt(x, wav, n_iter=n_iter, interp=interp)
        out[(n_iter, interp)] = M.share(Tx, f, ssq_freqs)
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(M.SIGNALS))
def test_sharpening(S, name, dtype):
    """The FM tone (period 300, N = 2048, gmw and Morlet mu = 13.4) and the linear chirp 0.05 -> 0.35 (N = 512, gmw):
    the share of ``|Tx|^2`` within +-1 bin of the true frequency grows strictly from 1 to 2 to 5 passes, does not fall
    from 5 to 10 by more than `SLACK`, the nearest-row form at 10 passes lies strictly between 1 pass and the linear
    form at 10, and every share is within `SHARE_MARGIN` of the NumPy float64 restatement's."""
    s = shares(S, name, dtype)
    ref = M.np_shares(name)
    lin = [s[(m, 'linear')] for m in (1, 2, 5, 10)]
    diff = {('%d_%s' % k): s[k] - ref[k] for k in M.PASSES}
    report_measured('msst_cwt_shares_%s_%s' % (name, dtype), one=lin[0], two=lin[1], five=lin[2], ten=lin[3],
                    ten_nearest=s[(10, 'nearest')], max_abs_diff_to_numpy=max(abs(v) for v in diff.values()))
    assert lin[0] < lin[1] < lin[2], lin
    assert lin[3] >= lin[2] - SLACK, lin
    assert lin[0] < s[(10, 'nearest')] < lin[3], (lin, s[(10, 'nearest')])
    for k, d in diff.items():
        assert abs(d) <= SHARE_MARGIN[dtype], (k, d, diff)
