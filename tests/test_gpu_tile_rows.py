# -*- coding: utf-8 -*-
"""The column-tile kernels of the fused `ssq_cwt` BY ROW COUNT: which kernel a scale vector of `na` rows
gets, and every build of the two that the suite ran at one shape only -- the 16-column float64 tile
(`tile2_kernel<.., COLS = 16>`, 320 .. 511 rows) and the 32-column tile with a column per lane
(`tile2_kernel<.., COLS = 32>`, the route when the pair kernel is not planned).

The boundaries, from the code (csrc/ssq_tiles.h, csrc/ssq_cwt_tiles.hip: a workgroup's tile of `na + 1` rows must
fit 160 KiB of LDS), derived here again and asserted on both sides:

    float64 tile, 32 columns   (na + 1) * 32 * 16     <= 163840   na <= 319    tile3_kernel (kernel 3; kernel 2 with
                                                                                SSQ_DEBUG_TILE_PAIR=0)
    float64 tile, 16 columns   (na + 1) * 16 * 16     <= 163840   na <= 639    tile2_kernel (kernel 2) for 320 .. 511
    ordered tile, 64 columns   (na + 1) * 64 * 8 + 16 <= 163840   na <= 318    tile_kernel (kernel 1); beyond: none
    packed row field, 9 bits   na < NA_MAX = 512                               512 rows and more: no tile plan, the
                                                                                block kernels + the separate reassignment

Inputs: `two_chirps` of N = 4201 (odd; its left padding n1 = 1996 is EVEN, the padded length 8192) and of N = 4118
(even; n1 = 2037 is ODD, so the pair kernel's tiles start a column early; 4118 = 4112 + 6: the last 16-column tile
holds 6 columns, the last 32-column one 22). 4201 leaves 9 columns to the last 16- and 32-column tiles. `gmw`
float32; `na` log-spaced scales between the ends of `process_scales('log', N, wav, nv=16)`; three signals per call.

Tolerances are the project's: 1e-5 `relmax` for `Wx`, `dWx` against the oracle's full-length transform;
`assert_tx_vs_oracle` for `Tx` against the oracle's reassignment of the device's own `Wx`, `dWx`;
`assert_tx_repeat` between two runs; `array_equal` for `Wx`, `dWx` and bin indices. Every statement about a route
reads a plan fact: `plan.tile_kernel`, `plan.tile_cols`, `plan.tiles_done()`, the grid integer and the weight
vector that reached `set_ssq`. tests/test_tile_rows_emulated.py runs a subset over the CPU emulation of the kernels;
profiles/tile_rows.txt has the measured figures and the mutations these tests catch.
"""
import os
import numpy as np
import pytest
from conftest import (two_chirps, assert_tx_vs_oracle, assert_tx_repeat, needs_tile_path, tile_mode,  # noqa: F401
                      tile_order, report_measured)
from pipeline import oracle_ssq_cwt, GRIDNAME
from test_gpu_transforms import relmax

pytestmark = pytest.mark.gpu

NS = (4201, 4118)
NAS = (63, 64, 65, 256, 318, 319, 320, 321, 383, 384, 385, 448, 511, 512)   # (318: the ordered kernel's last)
LDS_BYTES = 160 * 1024
GRID_INT = {'log': 0, 'log-piecewise': 1, 'linear': 2}
WEIGHTS = ('scalar', 'vec32', 'vec64')
GAMMA = 10 * float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()
    _CASE.clear()


def f64_tile_rows(cols):
    """most rows of a float64 tile of `cols` columns: `tile2_lds_bytes(na, cols) <= 160 KiB`"""
    return LDS_BYTES // (cols * 16) - 1


def ordered_tile_rows():
    """most rows of the ordered kernel's tile: `tile_lds_bytes(na) = (na + 1) * 64 * 8 + 16 <= 160 KiB`"""
    return (LDS_BYTES - 16) // (64 * 8) - 1


def expected_route(na, mode, pair=True):
    """(tile_kernel, tile_cols) of a plan of `na` rows: the table of the module's docstring."""
    from ssqueezepy_amd._tiles import NA_MAX
    if na >= NA_MAX:
        return 0, 0
    if mode == 'ordered':
        return (1, 64) if na <= ordered_tile_rows() else (0, 0)
    if na <= f64_tile_rows(32):
        return (3, 32) if pair else (2, 32)
    assert na <= f64_tile_rows(16)
    return 2, 16


def test_row_limits_are_the_documented_ones():
    """319 / 318 / 511: the numbers the comments and DESIGN.md state, from the LDS formulas."""
    from ssqueezepy_amd._tiles import NA_MAX
    assert f64_tile_rows(32) == 319 and ordered_tile_rows() == 318 and f64_tile_rows(16) >= NA_MAX - 1 == 511
    assert expected_route(319, 'f64') == (3, 32) and expected_route(320, 'f64') == (2, 16)
    assert expected_route(318, 'ordered') == (1, 64) and expected_route(319, 'ordered') == (0, 0)


def log_scales(N, na, wav):
    from ssqueezepy_amd.scales import process_scales
    s = np.asarray(process_scales('log', N, wav, nv=16), dtype='float64').reshape(-1)
    return np.exp(np.linspace(np.log(s[0]), np.log(s[-1]), na)).astype('float32')


def piecewise_scales(N, na, wav):
    """`na` scales over the same range in two exponential pieces, the upper half at half the rate -- what
    `process_scales('log-piecewise', ..)` makes, with a chosen row count (`infer_scaletype` -> 'log-piecewise')."""
    from ssqueezepy_amd.scales import process_scales
    s = np.asarray(process_scales('log', N, wav, nv=16), dtype='float64').reshape(-1)
    n_a = na // 2
    d = np.log(s[-1] / s[0]) / ((n_a - 1) + 2 * (na - n_a))
    lg = np.concatenate([np.arange(n_a) * d, (n_a - 1) * d + 2 * d * np.arange(1, na - n_a + 1)])
    return np.exp(np.log(s[0]) + lg).astype('float32')


_CASE = {}


def make_case(orc, N, na, nsig, kind='log'):
    """Signals, scales and the oracle's `Wx`, `dWx` (and, for 'log' scales, its design) per signal; the last
    few made are kept, so the two tile modes and the weight kinds of one shape share one reference."""
    key = (N, na, nsig, kind)
    if key in _CASE:
        return _CASE[key]
    while len(_CASE) >= 3:
        _CASE.pop(next(iter(_CASE)))
    from ssqueezepy_amd.wavelets import Wavelet
    wav = Wavelet(('gmw', {'dtype': 'float32'}))
    sc = (piecewise_scales if kind == 'log-piecewise' else log_scales)(N, na, wav)
    assert len(sc) == na
    x = np.stack([two_chirps(N, seed=N + 7 * s) for s in range(nsig)])
    r = [oracle_ssq_cwt(orc, x[s], 'float32', scales=sc, ssq=(s == 0 and kind == 'log')) for s in range(nsig)]
    for q in r:
        q.pop('Tx', None)
        q['Wx'].setflags(write=False), q['dWx'].setflags(write=False)
    _CASE[key] = dict(N=N, na=na, x=x, sc=sc, r=r)
    return _CASE[key]


def tiles_per_signal(N, kernel, cols):
    from ssqueezepy_amd.padding import pad_geometry
    if not cols:
        return 0
    lead = (pad_geometry(N)[1] & 1) if kernel == 3 else 0      # (the pair kernel starts a column early when n1 is odd)
    return -(-(N + lead) // cols)


def the_plan():
    from ssqueezepy_amd import _cwt
    assert len(_cwt._PLAN_CACHE) == 1, len(_cwt._PLAN_CACHE)
    return next(iter(_cwt._PLAN_CACHE.values()))


def check_rows(S, orc, N, na, nsig=3):
    """(a): the fused call at `na` rows in the mode the environment selects."""
    needs_tile_path()
    from ssqueezepy_amd import _cwt
    mode = tile_order()
    c = make_case(orc, N, na, nsig)
    x, sc, r0 = c['x'], c['sc'], c['r'][0]
    xb = x if nsig > 1 else x[0]
    one = min(1, nsig - 1)
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    kernel, cols = expected_route(na, mode)
    _cwt.clear_plan_cache()
    try:
        Tx, Wx, sf, scales, dWx = S.ssq_cwt(xb, wav, scales=sc, get_dWx=True, astensor=False)
        plan = the_plan()
        assert plan.na == na
        # what will run, and after the calls what ran
        assert (plan.tile_kernel, plan.tile_cols) == (kernel, cols), (plan.tile_kernel, plan.tile_cols, plan.algo)
        tps = tiles_per_signal(N, kernel, cols)
        assert plan.tiles_per_signal(N) == tps
        assert plan.tiles_done() == nsig * tps, (plan.tiles_done(), tps)
        if cols:
            assert plan.tile_rows > 0.5 * na, plan.tile_rows
        Tl, Wl, *_ = S.ssq_cwt(xb, wav, scales=sc, astensor=False)                      # the lean build
        T1, W1, _, _, dW1 = S.ssq_cwt(x[one], wav, scales=sc, get_dWx=True, astensor=False)
        assert the_plan() is plan
        assert plan.tiles_done() == (2 * nsig + 1) * tps, (plan.tiles_done(), tps)
    finally:
        _cwt.clear_plan_cache()
    assert np.array_equal(sf, r0['ssq_freqs']) and np.array_equal(scales, sc)
    assert r0['grid'] == GRID_INT['log']
    Tx, Wx, dWx, Tl, Wl = (a.reshape((nsig,) + a.shape[-2:]) for a in (Tx, Wx, dWx, Tl, Wl))
    eW = eD = eT = 0.0
    for s in range(nsig):
        r = c['r'][s]
        eW, eD = max(eW, relmax(Wx[s], r['Wx'])), max(eD, relmax(dWx[s], r['dWx']))
        ref = orc.ssqueeze(Wx[s], dWx[s], 'log', r0['params'], r0['const'], r0['gamma'], True, typing=0)
        eT = max(eT, assert_tx_vs_oracle(Tx[s], ref, tiles=True, what=(na, s)))
        assert_tx_repeat(Tl[s], Tx[s], what=('lean', na, s))
    report_measured('tile_rows', kernel=kernel, cols=cols, na=na, N=N, grid='log', weights='scalar', mode=mode,
                    Wx=eW, dWx=eD, Tx=eT)
    assert eW <= 1e-5 and eD <= 1e-5, (eW, eD)
    assert np.array_equal(Wl, Wx)
    # signal `one` of the batch against a call of its own
    assert np.array_equal(W1, Wx[one]) and np.array_equal(dW1, dWx[one])
    assert_tx_repeat(T1, Tx[one], what=('single', na))
    if nsig > 1:
        assert not np.array_equal(Wx[0], Wx[1])


@pytest.mark.parametrize('na', NAS)
@pytest.mark.parametrize('N', NS)
def test_tile_kernel_by_row_count(S, orc, N, na, tile_mode):
    """`na` rows around every number the row count decides -- multiples of the write-out round (64), 319 / 320
    (32- to 16-column tile), 318 / 319 (the ordered kernel's last / none), 511 / 512 (the last tile plan / the
    block route) -- for an odd and an even N, in both tile modes: the kernel and tile the plan reports, the tiles
    the kernel counted, `Wx`, `dWx`, `Tx` of every signal of a batch of three, the lean build against the full
    one, a signal of the batch against a call of its own. The ordered kernel runs up to 318 rows
    (`tile_lds_bytes`) and none beyond; at 512 rows no tile plan exists and the result is as right."""
    check_rows(S, orc, N, na)


def design_of(S, N, na, grid):
    """Scales and the host design for the frequency grid `grid`: 'log' and 'linear' over log-spaced scales
    ('linear' as `ssq_freqs='linear', maprange='maximal'`), 'log-piecewise' over piecewise SCALES (asked for
    as `ssq_freqs` over log-spaced scales it comes back as grid 0)."""
    from ssqueezepy_amd import _ssq_cwt
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    _ssq_cwt._DESIGN_CACHE.clear()
    if grid == 'linear':
        design = _ssq_cwt._ssq_design(wav, log_scales(N, na, wav), None, N, 1., 'linear', 'maximal', True)
    elif grid == 'log-piecewise':
        design = _ssq_cwt._ssq_design(wav, piecewise_scales(N, na, wav), None, N, 1., None, 'peak', True)
    else:
        design = _ssq_cwt._ssq_design(wav, log_scales(N, na, wav), None, N, 1., None, 'peak', True)
    return (wav,) + tuple(design)


def weights_of(kind, na):
    """one float32; a float32 per row; a float64 per row (the rows above 256 differ from those 256 below)"""
    if kind == 'scalar':
        return np.log(2) / 32
    v = np.log(2) / np.linspace(8, 32, na)
    return v.astype('float32') if kind == 'vec32' else v


def set_ssq_checked(plan, grid, gridname, params, const, weights, na):
    """`set_ssq`, and what reached the C ABI: the grid integer, the weight vector's size and dtype."""
    assert grid == GRID_INT[gridname], (grid, gridname)
    plan.set_ssq(grid, params, const, True, GAMMA)
    assert plan._ssq_key[0] == GRID_INT[gridname]
    sent = np.frombuffer(plan._ssq_key[2], dtype='float64' if weights == 'vec64' else 'float32')
    assert sent.size == na, (sent.size, na)
    assert (np.ptp(sent) == 0) == (weights == 'scalar')
    assert np.array_equal(sent, np.broadcast_to(np.asarray(const, dtype=sent.dtype), (na,)))


def check_build(S, orc, N, na, gridname, weights, pair=True, nsig=3):
    """(b), (c): one (grid, weights) build of the float64-tile kernel, with `dWx` stored and lean, through
    the plan interface; `pair=False`: the column-per-lane kernel where the pair kernel would run."""
    needs_tile_path()
    if tile_order() == 'ordered':
        pytest.skip('the ordered mode runs the ticketed kernel (none beyond 318 rows)')
    import torch
    from ssqueezepy_amd import _cwt, algos
    kind = 'log-piecewise' if gridname == 'log-piecewise' else 'log'
    c = make_case(orc, N, na, nsig, kind)
    wav, scales_dt, ssq_freqs, _, grid, params = design_of(S, N, na, gridname)
    assert np.array_equal(scales_dt.reshape(-1), c['sc'])
    const = weights_of(weights, na)
    kernel, cols = expected_route(na, 'f64', pair)
    assert kernel == 2 or pair
    _cwt.clear_plan_cache()
    try:
        plan = _cwt.get_cwt_plan(wav, scales_dt, N, 'reflect', 1., True, nsig)
        set_ssq_checked(plan, grid, gridname, params, const, weights, na)
        assert (plan.tile_kernel, plan.tile_cols) == (kernel, cols), (plan.tile_kernel, plan.tile_cols, plan.algo)
        tps = tiles_per_signal(N, kernel, cols)
        xd = algos.to_device(c['x'] if nsig > 1 else c['x'][0], torch.float32)
        out = plan.execute(xd, want_dWx=True, want_Tx=True)
        Tx, Wx, dWx = (out[k].cpu().numpy().reshape(nsig, na, N) for k in ('Tx', 'Wx', 'dWx'))
        assert plan.tiles_done() == nsig * tps, (plan.tiles_done(), tps)
        out = plan.execute(xd, want_Tx=True)                                             # the lean build
        Tl, Wl = (out[k].cpu().numpy().reshape(nsig, na, N) for k in ('Tx', 'Wx'))
        assert plan.tiles_done() == 2 * nsig * tps, (plan.tiles_done(), tps)
        assert plan.tile_rows > 0.5 * na
    finally:
        _cwt.clear_plan_cache()
    eW = eD = eT = 0.0
    for s in range(nsig):
        r = c['r'][s]
        eW, eD = max(eW, relmax(Wx[s], r['Wx'])), max(eD, relmax(dWx[s], r['dWx']))
        ref = orc.ssqueeze(Wx[s], dWx[s], GRIDNAME[grid], params, const, GAMMA, True, typing=0)
        eT = max(eT, assert_tx_vs_oracle(Tx[s], ref, tiles=True, what=(gridname, weights, na, s)))
        assert_tx_vs_oracle(Tl[s], ref, tiles=True, what=('lean', gridname, weights, na, s))
        assert_tx_repeat(Tl[s], Tx[s], what=('lean', na, s))
    report_measured('tile_rows_build', kernel=kernel, cols=cols, na=na, N=N, grid=gridname, weights=weights,
                    Wx=eW, dWx=eD, Tx=eT)
    assert eW <= 1e-5 and eD <= 1e-5, (eW, eD)
    assert np.array_equal(Wl, Wx)


@pytest.mark.parametrize('weights', WEIGHTS)
@pytest.mark.parametrize('grid', list(GRID_INT))
@pytest.mark.parametrize('na', [320, 511])
@pytest.mark.parametrize('N', NS)
def test_16_column_tile_every_build(S, orc, N, na, grid, weights):
    """The 18 builds of `tile2_kernel<.., COLS = 16>` -- three frequency grids x three kinds of reassignment
    weight x (`dWx` stored, lean) -- at its first and its last row count: the grid integer and the weight
    vector that reached `set_ssq`, kernel 2 with 16 columns, the tile count, `Tx` of both builds against the
    oracle's reassignment with the same grid, parameters and weights."""
    check_build(S, orc, N, na, grid, weights)


@pytest.mark.parametrize('weights', WEIGHTS)
@pytest.mark.parametrize('grid', list(GRID_INT))
def test_single_column_32_tile_every_build(S, orc, grid, weights, monkeypatch, N=4201, na=319):
    """The same for `tile2_kernel<.., COLS = 32>` at its last row count, where `SSQ_DEBUG_TILE_PAIR=0` keeps it in
    the pair kernel's place (kernel 2, 32 columns)."""
    monkeypatch.setenv('SSQ_DEBUG_TILE_PAIR', '0')
    check_build(S, orc, N, na, grid, weights, pair=False)


def check_bins(S, orc, N, na, weights, nsig=3):
    """(d): every point's bin as the 16-column kernel consumed it (`plan.set_bin_dump`: the `STORE_K` twin of the
    build), lean and full, against the oracle's `get_k` map of the device's own `Wx`, `dWx`."""
    needs_tile_path()
    if tile_order() == 'ordered':
        pytest.skip("the ordered kernel's Tx is the CPU loop's bit for bit: its bins need no dump")
    import torch
    from ssqueezepy_amd import _cwt, algos
    c = make_case(orc, N, na, nsig)
    wav, scales_dt, ssq_freqs, _, grid, params = design_of(S, N, na, 'log')
    const = weights_of(weights, na)
    kernel, cols = expected_route(na, 'f64')
    _cwt.clear_plan_cache()
    try:
        plan = _cwt.get_cwt_plan(wav, scales_dt, N, 'reflect', 1., True, nsig)
        set_ssq_checked(plan, grid, 'log', params, const, weights, na)
        assert (plan.tile_kernel, plan.tile_cols) == (kernel, cols) == (2, 16)
        tps = tiles_per_signal(N, kernel, cols)
        xd = algos.to_device(c['x'] if nsig > 1 else c['x'][0], torch.float32)
        kmap = torch.full((plan.max_batch * na * N,), -2, dtype=torch.int16, device=algos.device())
        plan.set_bin_dump(kmap)
        try:
            out = plan.execute(xd, want_Tx=True)                                         # lean build
            k_lean = kmap[:nsig * na * N].cpu().numpy().view(np.uint16).reshape(nsig, na, N).copy()
            Wl = out['Wx'].cpu().numpy().reshape(nsig, na, N)
            kmap.fill_(-2)
            out = plan.execute(xd, want_dWx=True, want_Tx=True)                          # full build
            k_full = kmap[:nsig * na * N].cpu().numpy().view(np.uint16).reshape(nsig, na, N).copy()
            Tx, Wx, dWx = (out[k].cpu().numpy().reshape(nsig, na, N) for k in ('Tx', 'Wx', 'dWx'))
            assert plan.tiles_done() == 2 * nsig * tps, (plan.tiles_done(), tps)
        finally:
            plan.set_bin_dump(None)
    finally:
        _cwt.clear_plan_cache()
    unwritten = np.uint16(0xFFFE)                                                        # (-2: no point's bin)
    assert not (k_lean == unwritten).any() and not (k_full == unwritten).any()
    assert np.array_equal(Wl, Wx) and np.array_equal(k_lean, k_full)
    below = 0
    for s in range(nsig):
        ref, k_ref = orc.ssqueeze(Wx[s], dWx[s], 'log', params, const, GAMMA, True, typing=0, get_k=True)
        want = np.where(k_ref < 0, 0xFFFF, k_ref).astype(np.uint16)
        bad = int((k_full[s] != want).sum())
        assert bad == 0, (s, bad, np.argwhere(k_full[s] != want)[:5].tolist())
        assert_tx_vs_oracle(Tx[s], ref, tiles=True, what=('bins', weights, na, s))
        below += int((k_ref < 0).sum())
    report_measured('tile_rows_bins', kernel=kernel, cols=cols, na=na, N=N, grid='log', weights=weights,
                    points=int(k_full.size), below_gamma=below, mismatches=0)


@pytest.mark.parametrize('weights', ['scalar', 'vec64'])
@pytest.mark.parametrize('na', [320, 511])
def test_16_column_bins_are_the_oracles_integers(S, orc, na, weights, N=4201):
    """The 16-column kernel's index work as INTEGERS, as `test_config2_bin_indices_are_the_oracles_integers` has
    it for the 32-column pair kernel: every index `array_equal` to the oracle's map, no point left unwritten,
    the lean build's map equal to the full build's -- with one weight per transform and with a float64 per row
    (the build whose per-row weight is selected by the record's 9-bit row field)."""
    check_bins(S, orc, N, na, weights)
