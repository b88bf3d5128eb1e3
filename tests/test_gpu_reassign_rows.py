# -*- coding: utf-8 -*-
"""The reassignment kernels behind `launch_accumulate` (csrc/ssq_kernels.hip) BY ROW COUNT: every route of the rule
`ssq_reassign_route` answers, on both sides of every LDS edge, from every bin source -- `ssqueeze_fast` (bins from
dWx, with and without the bin map), `indexed_sum_onfly` (from a stored w), `indexed_sum_bins` (from a caller's map).

    route                                        float32 data        float64 data
    accumulate_tile16_kernel, 32 columns         na <= 320           -
    accumulate_tile16_kernel, 16 columns         321 .. 1280         <= 640
    accumulate_tile_kernel, 8 columns            1281 .. 2560        641 .. 1280
    accumulate_tile_kernel, 4 columns            2561 .. 5120        1281 .. 2560
    accumulate_global_kernel                     >= 5121             >= 2561
    accumulate_f64_kernel (bin map), 32/16/8     <= 160 / 640 / -    <= 160 / 640 / 1280

Every case asserts the route it means to test from the query first. References: the CPU oracle on inputs whose bins
spread over the grid (tests/reassign_rows.py: `spread_case`, the condition is asserted on the oracle's own bin map),
`ordered_sum` on crafted bin maps with integer planes (exact in any order) and with planes whose sums depend on the
order, `exact_sum` with the rounding bound of a float64 sum for the unordered kernel. Ordered routes are held to
`array_equal`; bins from a stored float32 `w` on the log grids also to the rule of
test_gpu_kernels.py::test_indexed_sum_onfly. tests/test_reassign_rows_emulated.py runs a subset over the CPU emulation;
profiles/reassign_rows.txt has the measured figures and the mutations these tests catch.
"""
import numpy as np
import pytest
from conftest import two_chirps, assert_tx_vs_oracle, assert_tx_repeat, report_measured
import reassign_rows as R

pytestmark = pytest.mark.gpu
DTYPES = ('float32', 'float64')


@pytest.fixture(scope='module')
def A():
    from conftest import compute_module
    for mod in compute_module():
        from ssqueezepy_amd import algos
        yield algos


def _np(t):
    return t.detach().cpu().numpy()


def set_order(mp, ordered):
    if ordered:
        mp.setenv('SSQ_TILE_ORDER', 'ordered')
    else:
        mp.delenv('SSQ_TILE_ORDER', raising=False)


def routed(A, dtype, src, na, n, ordered=False, kmap=False, want=None):
    """The route the library answers, which must be the rule's (and `want`, a (kernel, cols), where the case names one)."""
    got = A.reassign_route(dtype, src, na, n, ordered=ordered, kmap=kmap)
    assert got == R.route(dtype, src, na, n, ordered, kmap), (got, dtype, src, na, n)
    assert want is None or got[:2] == tuple(want), (got, want)
    return got


def assert_f64_sum(out, Wx, k, const, what=''):
    """A result of the unordered float64 tile against the exact sum: a cell without terms exactly +0, else within the
    rounding bound of a float64 sum in any order (plus the one rounding to float32). -> largest error / bound"""
    m, S, Ab = R.exact_sum(Wx, k, const)
    worst = 0.0
    for part, s, a in zip((out.real, out.imag), S, Ab):
        empty = m == 0
        assert not part[empty].any() and not np.signbit(part[empty]).any(), what
        err = np.abs(part.astype(np.longdouble) - s)
        bound = R.f64_sum_bound(Wx.real.dtype, m, s, a)
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, np.longdouble(1e-300))).max()))
        live = bound > 0
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
    return worst


# --------------------------------------------------------------------------------------------------- row count
def check_rows(A, orc, dtype, na, mp, n=None, grids=R.GRIDS, weights=R.WEIGHTS):
    n = n or R.columns_for(na)
    want = routed(A, dtype, 'dwx', na, n)
    assert routed(A, dtype, 'dwx', na, n, kmap=True) == want == routed(A, dtype, 'w', na, n)
    assert routed(A, dtype, 'bins', na, n, ordered=True) == want
    unordered = routed(A, dtype, 'bins', na, n)
    assert (unordered[0] == 'f64') == (na <= R.F64_LIMITS[dtype][-1])
    worst = 0.0
    for gi, grid in enumerate(grids if na > 2 else ('linear',)):
        c = R.spread_case(dtype, na, n, grid)
        Wx, dWx, sf, gamma = c['Wx'], c['dWx'], c['sf'], c['gamma']
        logscale = grid.startswith('log')
        p = R.grid_params(sf, grid)
        w = R.w_plane(orc, c)
        for wi, kind in enumerate(weights):
            flipud = (gi + wi) % 2 == 1
            const = R.weight(kind, na, dtype)
            what = (dtype, na, grid, kind, flipud)
            ref, kref = orc.ssqueeze(Wx, dWx, grid, p, const, gamma, flipud, typing=0, get_k=True)
            hit, top = R.spread_ok(kref, na)
            assert hit >= 0.9 and top <= R.spread_bound(na), (what, hit, top)
            # bins from dWx, with the bin map and without
            set_order(mp, False)
            out, k = A.ssqueeze_fast(Wx, dWx, sf, const, logscale, flipud, gamma, get_k=True)
            assert np.array_equal(_np(k), kref), what
            assert np.array_equal(_np(out), ref), what
            assert np.array_equal(_np(A.ssqueeze_fast(Wx, dWx, sf, const, logscale, flipud, gamma)), ref), what
            # bins from a stored w
            refw = orc.indexed_sum(Wx, w, grid, p, const, flipud, typing=0)
            outw = _np(A.indexed_sum_onfly(Wx, w, sf, const, logscale, flipud))
            # (float32 log grids too: the kernel takes log2 of a stored float32 w with glibc's bits, `log2f_cpu_bits`;
            # the reference's looser rule for them is held in `test_stored_w_on_float32_log_grids`)
            assert np.array_equal(outw, refw), what
            # bins from the oracle's map: the unordered float64 tile where it fits, and the ordered kernels
            kmap = R.to_map(kref)
            outb = _np(A.indexed_sum_bins(Wx, kmap, const))
            if unordered[0] == 'f64':
                worst = max(worst, assert_f64_sum(outb, Wx, kref, const, what))
            else:
                assert np.array_equal(outb, ref), what
            set_order(mp, True)
            assert np.array_equal(_np(A.indexed_sum_bins(Wx, kmap, const)), ref), what
            set_order(mp, False)
    if na > 2:
        # the STFT form of w, on the rows' own linear grid
        c = R.spread_case(dtype, na, n, 'linear', stft=True)
        p = R.grid_params(c['sf'], 'linear')
        for wi, kind in enumerate(weights):
            const = R.weight(kind, na, dtype)
            ref, kref = orc.ssqueeze(c['Wx'], c['dWx'], 'linear', p, const, c['gamma'], wi % 2 == 1, Sfs=c['Sfs'], typing=0,
                                     get_k=True)
            hit, top = R.spread_ok(kref, na)
            assert hit >= 0.9 and top <= R.spread_bound(na), (na, 'stft', hit, top)
            out, k = A.ssqueeze_fast(c['Wx'], c['dWx'], c['sf'], const, False, wi % 2 == 1, c['gamma'], Sfs=c['Sfs'],
                                     get_k=True)
            assert np.array_equal(_np(k), kref) and np.array_equal(_np(out), ref), (dtype, na, 'stft', kind)
    return want, unordered, worst


def check_stored_w_log(A, orc, na, n=None):
    """Bins from a stored float32 `w` on the two log grids, the rule of test_gpu_kernels.py::test_indexed_sum_onfly:
    mean |diff| < 1e-8 and fewer than 1e-3 of the cells differ. -> the largest of each"""
    n = n or R.columns_for(na)
    routed(A, 'float32', 'w', na, n)
    worst = [0.0, 0.0, 0]
    for gi, grid in enumerate(('log-piecewise', 'log')):
        c = R.spread_case('float32', na, n, grid)
        p = R.grid_params(c['sf'], grid)
        w = R.w_plane(orc, c)
        for wi, kind in enumerate(('scalar', 'vec64')):
            flipud = (gi + wi) % 2 == 1
            const = R.weight(kind, na, 'float32')
            ref = orc.indexed_sum(c['Wx'], w, grid, p, const, flipud, typing=0)
            out = _np(A.indexed_sum_onfly(c['Wx'], w, c['sf'], const, True, flipud))
            mean, frac = float(np.abs(out - ref).mean()), float((out != ref).mean())
            print('stored w, float32:', na, grid, kind, flipud, 'mean |diff| %.3g' % mean, 'cells that differ %.3g' % frac,
                  '=', int((out != ref).sum()))
            worst = [max(worst[0], mean), max(worst[1], frac), max(worst[2], int((out != ref).sum()))]
    return worst


@pytest.mark.parametrize('na', [na for na in R.NAS['float32'] if na > 2])
def test_stored_w_on_float32_log_grids(A, orc, na):
    """`indexed_sum_onfly` on float32 log grids at every row count, held to the rule the reference states for it and
    test_gpu_kernels.py::test_indexed_sum_onfly keeps at 100 rows: mean |diff| < 1e-8, fewer than 1e-3 of the cells
    differ. One moved point among 1e5 cells is a mean of 6e-7, so at these sizes the rule allows none. With the device
    library's log2f it was missed from 1280 rows on (mean |diff| 9.0e-7 at 1280 rows, 2 cells of 89600, to 1.7e-5 at
    5121 rows, 46 cells of 230445: points whose log2 lies within an ulp of a bin edge, of which a grid of `na` rows has
    `na` times as many); `log2f_cpu_bits` (csrc/ssq_point_math.inl) now takes that logarithm with glibc's bits."""
    mean, frac, cells = check_stored_w_log(A, orc, na)
    report_measured('reassign_rows_w_plane', na=na, mean_abs_diff=mean, cells_that_differ=frac, count=cells)
    assert mean < 1e-8, (na, mean, cells)
    assert frac < 1e-3, (na, frac)


@pytest.mark.parametrize('dtype,na', [(d, na) for d in DTYPES for na in R.NAS[d]])
def test_every_route_by_row_count(A, orc, dtype, na, monkeypatch):
    """`na` at the RL and RL * U steps of each build and on both sides of every LDS edge; every bin source, the three
    grids, both `flipud`, the three weight kinds at every `na`, the STFT form on the linear grid. Bins and sums of the
    ordered routes bit for bit; the unordered float64 tile within the rounding bound of its sum."""
    want, unordered, worst = check_rows(A, orc, dtype, na, monkeypatch)
    report_measured('reassign_rows', dtype=dtype, na=na, route='%s/%d' % want[:2], bins_route='%s/%d' % unordered[:2],
                    f64_err_over_bound=worst)


# --------------------------------------------------------------------------------------------------- column count
def column_counts(kernel, cols):
    TC = 256 if kernel == 'global' else cols          # (the global kernel: 256 columns per workgroup, no tile order)
    if kernel == 'global':
        return (1, TC - 1, TC, TC + 1)
    return (1, TC - 1, TC, TC + 1, 8 * TC - 1, 8 * TC + 1, 9 * TC + 3)


def first_rows(dtype, kernel, cols):
    return [lo for (d, k, c, _), (lo, hi) in R.BUILDS.items() if (d, k, c) == (dtype, kernel, cols)][0]


def check_columns(A, orc, dtype, kernel, cols, mp, ns=None, src_kinds=('dwx', 'w', 'bins')):
    """A batch of three signals that differ, each against a call of its own, at column counts around the tile and
    around eight tiles (the XCD remap of the tile order and the early return). `na`: the first row count of the build
    -- the columns' arithmetic does not depend on it -- but past one step of the build."""
    na = max(first_rows(dtype, kernel, cols), 37)
    f64cols = R.route(dtype, 'bins', na, 1)
    for n in ns or column_counts(kernel, cols):
        routed(A, dtype, 'dwx', na, n, want=(kernel, cols))
        grid = R.GRIDS[n % 3]
        cs = [R.spread_case(dtype, na, n, grid, seed=s + 1) for s in range(3)]
        sf, p = cs[0]['sf'], R.grid_params(cs[0]['sf'], grid)
        Wb, dWb = np.stack([c['Wx'] for c in cs]), np.stack([c['dWx'] for c in cs])
        assert not np.array_equal(Wb[0], Wb[1])
        const = R.weight(R.WEIGHTS[n % 3], na, dtype)
        logscale = grid.startswith('log')
        set_order(mp, False)
        outb, kb = A.ssqueeze_fast(Wb, dWb, sf, const, logscale, True, R.GAMMA, get_k=True)
        outb, kb = _np(outb), _np(kb)
        wb = np.stack([R.w_plane(orc, c) for c in cs])
        outw = _np(A.indexed_sum_onfly(Wb, wb, sf, const, logscale, True)) if 'w' in src_kinds else None
        for s in range(3):
            ref, kref = orc.ssqueeze(Wb[s], dWb[s], grid, p, const, R.GAMMA, True, typing=0, get_k=True)
            assert np.array_equal(kb[s], kref) and np.array_equal(outb[s], ref), (n, s)
            o1, k1 = A.ssqueeze_fast(Wb[s], dWb[s], sf, const, logscale, True, R.GAMMA, get_k=True)
            assert np.array_equal(_np(o1), outb[s]) and np.array_equal(_np(k1), kb[s]), (n, s)
            if outw is not None:
                assert np.array_equal(_np(A.indexed_sum_onfly(Wb[s], wb[s], sf, const, logscale, True)), outw[s]), (n, s)
        if 'bins' in src_kinds:
            km = R.to_map(kb)
            set_order(mp, True)
            routed(A, dtype, 'bins', na, n, ordered=True, want=(kernel, cols))
            ob = _np(A.indexed_sum_bins(Wb, km, const))
            assert np.array_equal(ob, outb), n
            set_order(mp, False)


BUILD_IDS = [(d, k, c) for (d, k, c, _) in R.BUILDS]


@pytest.mark.parametrize('dtype,kernel,cols', BUILD_IDS)
def test_column_count_on_every_build(A, orc, dtype, kernel, cols, monkeypatch):
    """n = 1, TC - 1, TC, TC + 1, 8 TC - 1, 8 TC + 1, 9 TC + 3 on each of the nine ordered builds, a batch of three:
    every signal bit for bit its single call and the oracle."""
    check_columns(A, orc, dtype, kernel, cols, monkeypatch)


def check_f64_columns(A, orc, dtype, cols, mp, ns=None):
    lo, hi = R.F64_BUILDS[(dtype, cols)]
    na = max(lo, 37)
    for n in ns or column_counts('f64', cols):
        routed(A, dtype, 'bins', na, n, want=('f64', cols))
        grid = R.GRIDS[n % 3]
        cs = [R.spread_case(dtype, na, n, grid, seed=s + 1) for s in range(3)]
        p = R.grid_params(cs[0]['sf'], grid)
        const = R.weight(R.WEIGHTS[n % 3], na, dtype)
        Wb = np.stack([c['Wx'] for c in cs])
        ks = [orc.ssqueeze(c['Wx'], c['dWx'], grid, p, const, R.GAMMA, True, typing=0, get_k=True)[1] for c in cs]
        km = R.to_map(np.stack(ks))
        set_order(mp, False)
        ob = _np(A.indexed_sum_bins(Wb, km, const))
        for s in range(3):
            assert_f64_sum(ob[s], Wb[s], ks[s], const, (n, s))
            o1 = _np(A.indexed_sum_bins(Wb[s], km[s], const))
            assert_tx_repeat(o1, ob[s], tiles=True, what=(n, s))


@pytest.mark.parametrize('dtype,cols', list(R.F64_BUILDS))
def test_column_count_on_the_unordered_tile(A, orc, dtype, cols, monkeypatch):
    """The same column counts on the five builds of `accumulate_f64_kernel`: every signal of the batch within the
    float64 sum's bound and `assert_tx_repeat` against its single call."""
    check_f64_columns(A, orc, dtype, cols, monkeypatch)


# --------------------------------------------------------------------------------------------------- crafted maps
def last_rows(dtype, kernel, cols):
    lo, hi = [v for (d, k, c, _), v in R.BUILDS.items() if (d, k, c) == (dtype, kernel, cols)][0]
    return hi or lo


def check_patterns(A, orc, dtype, kernel, cols, mp, n=None, names=R.PATTERN_NAMES, na=None):
    """Crafted bin maps at the row count just below the build's upper edge (the global kernel: its first), as a bin
    map, as ``w = ssq_freqs[k]`` and as ``dWx = Wx 2 pi i ssq_freqs[k]`` on the linear grid: integer planes against the
    exact result, order-sensitive planes against `ordered_sum` -- which differs on reversed rows."""
    na = na or last_rows(dtype, kernel, cols)
    n = n or (2 * cols + 3 if kernel != 'global' else 11)
    for src in R.BINSRCS:
        routed(A, dtype, src, na, n, ordered=True, want=(kernel, cols))
    sf = R.make_ssq_freqs(na, 'linear')
    Wi, wi = R.int_plane(dtype, na, n)
    Ww = R.wide_plane(dtype, na, n)
    P = R.patterns(na, n)
    reversed_differs = set()

    def every_source(Wx, k, const, ref, what):
        w, dWx, Wz = R.pattern_planes(Wx, k, sf)
        set_order(mp, True)
        assert np.array_equal(_np(A.indexed_sum_bins(Wx, R.to_map(k), const)), ref), what + ('bins',)
        set_order(mp, False)
        assert np.array_equal(_np(A.indexed_sum_onfly(Wx, w, sf, const, False, False)), ref), what + ('w',)
        out, kd = A.ssqueeze_fast(Wz, dWx, sf, const, False, False, R.PATTERN_GAMMA, get_k=True)
        assert np.array_equal(_np(kd), k), what + ('the bins of dWx',)
        assert np.array_equal(_np(out), ref), what + ('dwx',)

    for pi, name in enumerate(names):
        k = P[name]
        exact = R.ordered_sum(Wi, k, wi)
        every_source(Wi, k, wi, exact, (name, 'int'))
        kind = R.WEIGHTS[::-1][pi % 3]                      # vec64 first: `weighted_add`'s float64 product
        const = R.weight(kind, na, dtype)
        ref = R.ordered_sum(Ww, k, const)
        every_source(Ww, k, const, ref, (name, 'wide', kind))
        c = np.asarray(const)
        rev = R.ordered_sum(Ww[::-1], k[::-1], c[::-1] if c.size == na else const)
        if not np.array_equal(rev, ref):
            reversed_differs.add(name)
    assert reversed_differs >= set(names) - set(R.ORDER_FREE), reversed_differs


@pytest.mark.parametrize('dtype,kernel,cols', BUILD_IDS)
def test_crafted_maps_on_every_build(A, orc, dtype, kernel, cols, monkeypatch):
    check_patterns(A, orc, dtype, kernel, cols, monkeypatch)


def check_f64_kernel(A, orc, dtype, cols, mp, n=None, names=R.PATTERN_NAMES):
    """`accumulate_f64_kernel` through `indexed_sum_bins` at the last row count of a build: crafted maps with integer
    planes (exact) and order-sensitive planes (the float64 sum's bound per cell), a spread random map likewise; then the
    same maps in the ordered mode against `ordered_sum`."""
    lo, na = R.F64_BUILDS[(dtype, cols)]
    n = n or 2 * cols + 3
    routed(A, dtype, 'bins', na, n, want=('f64', cols))
    routed(A, dtype, 'bins', na, n, ordered=True, want=R.route(dtype, 'dwx', na, n)[:2])
    Wi, wi = R.int_plane(dtype, na, n)
    Ww = R.wide_plane(dtype, na, n)
    P = R.patterns(na, n)
    c = R.spread_case(dtype, na, n, 'log')
    _, kspread = orc.ssqueeze(c['Wx'], c['dWx'], 'log', R.grid_params(c['sf'], 'log'), 1., R.GAMMA, True, typing=0,
                              get_k=True)
    hit, top = R.spread_ok(kspread, na)
    assert hit >= 0.9 and top <= R.spread_bound(na)
    worst = 0.0
    for pi, (name, k) in enumerate([(nm, P[nm]) for nm in names] + [('spread', kspread)]):
        km = R.to_map(k)
        kind = R.WEIGHTS[::-1][pi % 3]
        const = R.weight(kind, na, dtype)
        set_order(mp, False)
        assert np.array_equal(_np(A.indexed_sum_bins(Wi, km, wi)), R.ordered_sum(Wi, k, wi)), (name, 'int')
        worst = max(worst, assert_f64_sum(_np(A.indexed_sum_bins(Ww, km, const)), Ww, k, const, (name, 'wide', kind)))
        set_order(mp, True)
        assert np.array_equal(_np(A.indexed_sum_bins(Ww, km, const)), R.ordered_sum(Ww, k, const)), (name, 'ordered', kind)
        set_order(mp, False)
    return worst


@pytest.mark.parametrize('dtype,cols', list(R.F64_BUILDS))
def test_unordered_tile_against_the_exact_sum(A, orc, dtype, cols, monkeypatch):
    """|Tx - S| <= m 2^-53 A (float64 data), + 2^-24 (|S| + m 2^-53 A) (float32 data), per cell and part; a cell
    without terms is exactly +0: the rounding bounds of a float64 sum in any order, not measured values."""
    worst = check_f64_kernel(A, orc, dtype, cols, monkeypatch)
    report_measured('reassign_rows_f64_kernel', dtype=dtype, cols=cols, na=R.F64_BUILDS[(dtype, cols)][1],
                    err_over_bound=worst)


# --------------------------------------------------------------------------------------------------- out=
def check_out(A, orc, dtype, na, mp, n=19):
    import torch
    cdt = torch.complex64 if dtype == 'float32' else torch.complex128
    Wx = R.wide_plane(dtype, na, n)
    k = R.patterns(na, n)['gaps']                   # most cells stay empty
    sf = R.make_ssq_freqs(na, 'linear')
    w, dWx, Wz = R.pattern_planes(Wx, k, sf)
    ref = R.ordered_sum(Wx, k, 0.5)

    def nan_out():
        return A.to_device(np.full((na, n), np.nan + 1j * np.nan)).to(cdt)

    for ordered in (False, True):
        set_order(mp, ordered)
        routed(A, dtype, 'bins', na, n, ordered=ordered)
        for call in (lambda o: A.indexed_sum_bins(Wx, R.to_map(k), 0.5, out=o),
                     lambda o: A.indexed_sum_onfly(Wx, w, sf, 0.5, False, False, out=o),
                     lambda o: A.ssqueeze_fast(Wz, dWx, sf, 0.5, False, False, R.PATTERN_GAMMA, out=o)):
            o = nan_out()
            assert call(o) is o
            got = _np(o)
            assert not np.isnan(got.real).any() and not np.isnan(got.imag).any(), (na, ordered)
            if ordered or R.route(dtype, 'bins', na, n)[0] != 'f64':
                assert np.array_equal(got, ref), (na, ordered)
            empty = np.ones((na, n), bool)
            ii, jj = np.nonzero(k >= 0)
            empty[k[ii, jj], jj] = False
            assert not got[empty].any(), (na, ordered)
    set_order(mp, False)


@pytest.mark.parametrize('dtype,na', [('float32', 160), ('float32', 320), ('float32', 640), ('float32', 1280),
                                      ('float32', 2560), ('float32', 5120), ('float32', 5121),
                                      ('float64', 160), ('float64', 640), ('float64', 1280), ('float64', 2560),
                                      ('float64', 2561)])
def test_out_is_fully_overwritten(A, orc, dtype, na, monkeypatch):
    """A NaN-filled `out` on every route -- the nine ordered builds and the five of the unordered tile -- comes back
    without a NaN, empty cells 0: the tiles' write-out of empty cells and the global kernel's memset."""
    check_out(A, orc, dtype, na, monkeypatch)


# --------------------------------------------------------------------------------------------------- through the transforms
@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


CWT_CASES = [('float64', 160, ('f64', 32)), ('float64', 161, ('f64', 16)), ('float64', 641, ('f64', 8)),
             ('float64', 1281, ('tile', 4)), ('float32', 641, ('tile16', 16)), ('float32', 1281, ('tile', 8))]


def check_ssq_cwt(S, A, orc, dtype, na, want, N=2003):
    from pipeline import oracle_ssq_cwt
    from test_gpu_transforms import relmax
    from ssqueezepy_amd import _cwt
    x = two_chirps(N, seed=na)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    from ssqueezepy_amd.scales import process_scales
    s0 = np.asarray(process_scales('log', N, wav, nv=16), dtype='float64').reshape(-1)
    sc = np.exp(np.linspace(np.log(s0[0]), np.log(s0[-1]), na)).astype(dtype)     # `na` log-spaced scales over nv = 16's range
    r = oracle_ssq_cwt(orc, x, dtype, scales=sc)
    _cwt.clear_plan_cache()
    try:
        Tx, Wx, sf, scales, dWx = S.ssq_cwt(x, wav, scales=sc, get_dWx=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.na == na and Wx.shape == (na, N)
    finally:
        _cwt.clear_plan_cache()
    # float64 plans and float32 banks outside the column-tile plan reassign from the plan's bin map
    got = routed(A, dtype, 'bins', na, N, want=want)
    tol = 1e-5 if dtype == 'float32' else 1e-12
    assert relmax(Wx, r['Wx']) <= tol and relmax(dWx, r['dWx']) <= tol, (relmax(Wx, r['Wx']), relmax(dWx, r['dWx']))
    from pipeline import GRIDNAME
    ref = orc.ssqueeze(Wx, dWx, GRIDNAME[r['grid']], r['params'], r['const'], r['gamma'], True, typing=0)
    err = assert_tx_vs_oracle(Tx, ref, tiles=(got[0] == 'f64'), what=(dtype, na))
    return err


@pytest.mark.parametrize('dtype,na,want', CWT_CASES)
def test_ssq_cwt_reaches_these_routes(S, A, orc, dtype, na, want, monkeypatch):
    """`ssq_cwt` with explicit log-spaced scales: float64 with 160, 161, 641 and 1281 rows (the three builds of the
    unordered tile and the ordered 4-column tile above it), float32 with 641 and 1281 rows (ordered kernels: bit for
    bit). The route is the query's at the plan's (na, N)."""
    monkeypatch.delenv('SSQ_TILE_ORDER', raising=False)
    err = check_ssq_cwt(S, A, orc, dtype, na, want)
    report_measured('reassign_rows_ssq_cwt', dtype=dtype, na=na, route='%s/%d' % want, Tx=err)


# --------------------------------------------------------------------------------------------------- refusals
def check_refusals(A):
    import torch
    na, n = 40, 21
    Wx = R.wide_plane('float32', na, n)
    k = R.patterns(na, n)['mod3']
    out = A.to_device(np.full((na, n), 7 + 7j, dtype=np.complex64))
    keep = _np(out).copy()
    for bad in (na, na + 1, 0x7FFF, 0x8000, 0xFFFE):
        km = R.to_map(k)
        km[na - 1, n - 1] = bad
        with pytest.raises(ValueError, match='bin'):
            A.indexed_sum_bins(Wx, km, 1., out=out)
    with pytest.raises(TypeError):
        A.indexed_sum_bins(Wx, k.astype(np.int32), 1., out=out)
    with pytest.raises(TypeError):
        A.indexed_sum_bins(Wx, torch.from_numpy(k.astype(np.int16)), 1., out=out)
    with pytest.raises(TypeError):
        A.indexed_sum_bins(Wx.real.copy(), R.to_map(k), 1., out=out)
    with pytest.raises(ValueError):
        A.indexed_sum_bins(Wx, R.to_map(k)[:, :-1].copy(), 1., out=out)
    with pytest.raises(ValueError):
        A.indexed_sum_bins(Wx, R.to_map(k).T.copy(), 1., out=out)
    with pytest.raises(ValueError):
        A.indexed_sum_bins(Wx, R.to_map(k), 1., out=out[:, :-1])
    assert np.array_equal(_np(out), keep)
    # the skip mark and the last bin are both accepted
    km = R.to_map(k)
    km[0, 0], km[1, 0] = R.SKIP, na - 1
    kk = k.copy()
    kk[0, 0], kk[1, 0] = -1, na - 1
    got = A.indexed_sum_bins(Wx, km, 1., out=out)
    assert got is out
    assert_f64_sum(_np(out), Wx, kk, 1.)


def test_indexed_sum_bins_refuses(A, monkeypatch):
    """A bin >= na, a wrong dtype and a wrong shape are refused before any launch; `out` is left as it was."""
    monkeypatch.delenv('SSQ_TILE_ORDER', raising=False)
    check_refusals(A)
