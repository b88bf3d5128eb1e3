# -*- coding: utf-8 -*-
"""The float32 CWT on long signals (padded length M = 2^19 .. 2^22): every length of the LDS FFT
kernels, the 1024- and 2048-point ones included, checked ROW BY ROW.

What these inputs reach (the factors as `BlockPlan::setup_exact`, `AnalyticFft::create` and
`TilePlan` derive them from the length; the tests derive them again and assert the plan facts
that say which route ran):

    N         M      exact passes B x A     analytic signal B x A     longest tile class
                     (exact_pass1/2)        (tilefft_four_kernel)     (B x A of TilePlan)
    300001    2^19   512 x 1024             1024 x 512                2^17 (512 x 256)
    600001    2^20   1024 x 1024            1024 x 1024               2^18 (512 x 512)
    1100001   2^21   1024 x 2048            2048 x 1024               2^19 (1024 x 512)
    2100001   2^22   2048 x 2048            2048 x 2048               2^20 (1024 x 1024)

NOT reached, by any plan these lengths admit: a 2048-point transform of the TILE plan. Its classes
are L = M / R with a decimation R >= R_MIN = 4 (_tiles.py), so L <= M / 4 = 2^20 while M <= 2^22,
and a class of 2^20 points splits 1024 x 1024; a 2048-point factor needs L >= 2^21, that is
M >= 2^23, where the four-step paths of the CWT decline and rocFFT takes over.
`test_no_tile_class_has_a_2048_point_factor` states this with the planner's own constants.
`tilefft_four_kernel` itself runs its 2048-point instantiation here through the analytic signal.

The metric. `relmax` divides by the maximum of the whole array, and the row cut by the Nyquist bin --
the row that runs on the four-step ("exact") kernels -- is 2e-3 .. 5e-3 of that maximum: an exact row
wrong by 0.2 % of its own size passes `relmax <= 1e-5`. So every exact row is also held to a bound
of its own, against a float64 statement of the same operation built from the float32 bank
(`pipeline.oracle_cwt_rows_float64`; a float64 WAVELET differs from the float32 bank by 3e-6 .. 6e-6
of a row and would hide everything):

    e_dev(i) = max |dev_i - ref64_i| / max |ref64_i|  <=  2 * e_orc(i),

`e_orc(i)` the same quantity for the float32 oracle's row (scipy's pocketfft in float32: a full-length
float32 FFT of the same product, the yardstick a float32 four-step FFT has to meet). Under the CPU
emulation of these kernels the ratio is 0.13 .. 0.77; the factor 2 is for contracted and packed
device arithmetic, not for errors. Rows continued past Nyquist and block rows carry the method's
designed truncation (`tail_tol`: DESIGN.md), 1e-6 .. 1e-5 of the row; they are measured and reported
here (profiles/long_signals.txt), not bounded per row.
"""
import numpy as np
import pytest
from conftest import two_chirps, report_measured, needs_tile_path, assert_tx_repeat
from pipeline import oracle_ssq_cwt, oracle_cwt_rows_float64, row_errors
from test_gpu_transforms import relmax, check_Tx

pytestmark = pytest.mark.gpu

NS = (300001, 600001, 1100001, 2100001)
#       N: (M, exact passes (B, A), analytic signal (B, A), longest tile class)
REACHES = {300001: (1 << 19, (512, 1024), (1024, 512), 1 << 17),
           600001: (1 << 20, (1024, 1024), (1024, 1024), 1 << 18),
           1100001: (1 << 21, (1024, 2048), (2048, 1024), 1 << 19),
           2100001: (1 << 22, (2048, 2048), (2048, 2048), 1 << 20)}
# rows: every second 'log' scale of nv = 4 -- 12 of them, 8 at the two longest lengths (the host
# references are what these tests cost). Rows 0 and 1 are the ones cut by Nyquist, the tile rows of
# the longest class follow within the first 8.
N_ROWS = {300001: 12, 600001: 12, 1100001: 8, 2100001: 8}
WORKERS = 16          # threads of the host references' FFTs (not sized by the machine's CPU count)


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def exact_factors(M):
    """(B, A) of `BlockPlan::setup_exact`: pass 1 runs B-point, pass 2 A-point transforms."""
    lm = M.bit_length() - 1
    A = 1 << ((lm + 1) // 2)
    return M // A, A


def four_step_factors(L):
    """(B, A) of `AnalyticFft::create` and of a `TilePlan` class of L >= 2^13 points."""
    lg = L.bit_length() - 1
    return 1 << ((lg + 1) // 2), 1 << (lg // 2)


_CASE = {}


def make_case(orc, N):
    """Signal, scales and host references of one length; the last one made is kept (the module's
    `case` fixture groups the tests by length, so each length is computed once).

    r: the float32 oracle of the reference's full-length algorithm (pocketfft), `ssq_freqs` and the
    reassignment's parameters with it; W64 / D64: the float64 statement of every row; e_orc: the
    float32 oracle's per-row errors against it, (2, na) for Wx and dWx."""
    if N in _CASE:
        return _CASE[N]
    _CASE.clear()
    from ssqueezepy_amd.wavelets import Wavelet
    from ssqueezepy_amd.scales import process_scales
    wav = Wavelet(('gmw', {'dtype': 'float32'}))
    sc = np.asarray(process_scales('log', N, wav, nv=4), dtype='float32').reshape(-1)[::2][:N_ROWS[N]]
    x = two_chirps(N, seed=N)
    r = oracle_ssq_cwt(orc, x, 'float32', scales=sc, workers=WORKERS)
    del r['Tx']
    W64, D64 = oracle_cwt_rows_float64(orc, x, sc, range(len(sc)), workers=WORKERS)
    e_orc = np.stack([row_errors(r['Wx'], W64), row_errors(r['dWx'], D64)])
    _CASE[N] = dict(N=N, x=x, sc=sc, r=r, W64=W64, D64=D64, e_orc=e_orc)
    return _CASE[N]


@pytest.fixture(scope='module', params=NS)
def case(request, orc):
    yield make_case(orc, request.param)
    _CASE.clear()


def test_no_tile_class_has_a_2048_point_factor():
    """The tile plan's longest admissible class at M = 2^22 is M / R_MIN = 2^20 points, 1024 x 1024:
    no plan of these lengths holds a 2048-point tile transform (see the module's docstring)."""
    from ssqueezepy_amd import _tiles
    for N, (M, _, _, lmax) in REACHES.items():
        assert M // _tiles.R_MIN >= lmax
        assert max(four_step_factors(M // _tiles.R_MIN)) <= 1024, N
    assert max(four_step_factors((1 << 22) // _tiles.R_MIN * 2)) == 2048


def check_cwt_rows(S, orc, case, ext, monkeypatch):
    from ssqueezepy_amd import _cwt
    N, x, sc, r = case['N'], case['x'], case['sc'], case['r']
    M, exact_ba, analytic_ba, _ = REACHES[N]
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    monkeypatch.setenv('SSQ_DEBUG_CWT_NYQ_EXT', ext)
    monkeypatch.delenv('SSQ_DEBUG_TILE_FFT', raising=False)
    _cwt.clear_plan_cache()
    try:
        Wx, scales, dWx = S.cwt(x, wav, scales=sc, derivative=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        # what executed: the exact rows on the four-step kernels of these factors, the continued row
        # (ext '1') over an analytic signal made by the four-step kernels of those
        n_exact = 1 if ext == '1' else 2
        assert plan.M == M and exact_factors(M) == exact_ba and four_step_factors(M) == analytic_ba
        assert plan.algo.startswith('blockzoom') and 'fourstep' in plan.algo, plan.algo
        assert plan.block_rows == len(sc) - n_exact, (plan.block_rows, plan.algo)
        assert plan.extended_rows == (1 if ext == '1' else 0), plan.extended_rows
    finally:
        _cwt.clear_plan_cache()
    assert np.array_equal(scales, sc)
    kinds = ['exact'] * n_exact + ['continued'] * (2 - n_exact) + ['block'] * (len(sc) - 2)
    e_dev = np.stack([row_errors(Wx, case['W64']), row_errors(dWx, case['D64'])])
    e_orc = case['e_orc']
    for i, kind in enumerate(kinds):
        report_measured('long_cwt_rows', N=N, ext=ext, row=i, kind=kind,
                        Wx_dev=e_dev[0, i], Wx_orc=e_orc[0, i], dWx_dev=e_dev[1, i], dWx_orc=e_orc[1, i])
    # the project's contract, over the whole array
    eW, eD = relmax(Wx, r['Wx']), relmax(dWx, r['dWx'])
    assert eW <= 1e-5 and eD <= 1e-5, (eW, eD)
    # the exact rows, each against its own size
    for i in range(n_exact):
        for k, name in enumerate(('Wx', 'dWx')):
            assert e_dev[k, i] <= 2 * e_orc[k, i], (name, i, e_dev[k, i], e_orc[k, i])


@pytest.mark.parametrize('ext', ['1', '0'])
def test_cwt_rows_vs_float64_statement(S, orc, case, ext, monkeypatch):
    """`cwt` with its derivative at M = 2^19 .. 2^22, by default (row 0 exact: the gain limit refuses
    to continue it; row 1 continued past Nyquist) and with SSQ_DEBUG_CWT_NYQ_EXT=0 (rows 0 and 1
    exact): the plan facts, the 1e-5 contract against the float32 oracle, and every exact row
    against the float64 statement with the float32 oracle's own row error as the yardstick."""
    check_cwt_rows(S, orc, case, ext, monkeypatch)


def check_ssq_cwt_long(S, orc, case, lean=True):
    from ssqueezepy_amd import _cwt
    needs_tile_path()
    N, x, sc, r = case['N'], case['x'], case['sc'], case['r']
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    _cwt.clear_plan_cache()
    try:
        Tx, Wx, sf, scales, dWx = S.ssq_cwt(x, wav, scales=sc, get_dWx=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.tiles_done() == plan.tiles_per_signal(N) > 0
        lmax = int(plan.tile_plan['classes'][:, 0].max())
        assert lmax == REACHES[N][3], lmax
        tile_rows = np.nonzero(plan.tile_plan['interp_rows'])[0]
        if lean:          # the lean kernels (no `dWx` stored): exact_pass2_kernel<L, true> among them
            Tx_lean, Wx_lean, *_ = S.ssq_cwt(x, wav, scales=sc, astensor=False)
            assert np.array_equal(Wx_lean, Wx)
            assert_tx_repeat(Tx_lean, Tx)
    finally:
        _cwt.clear_plan_cache()
    assert np.array_equal(sf, r['ssq_freqs']) and np.array_equal(scales, sc)
    eW, eD = relmax(Wx, r['Wx']), relmax(dWx, r['dWx'])
    assert eW <= 1e-5 and eD <= 1e-5, (eW, eD)
    check_Tx(orc, Tx, Wx, dWx, r, 'float32')
    # the tile rows (interpolated from decimated samples), each against its own size
    assert len(tile_rows) > 0
    eWr, eDr = row_errors(Wx[tile_rows], r['Wx'][tile_rows]), row_errors(dWx[tile_rows], r['dWx'][tile_rows])
    for j, i in enumerate(tile_rows):
        report_measured('long_ssq_cwt_tile_rows', N=N, row=int(i), kind='tile',
                        L=int(REACHES[N][0] >> int(plan.tile_plan['lgR'][i])), Wx_vs_orc32=eWr[j], dWx_vs_orc32=eDr[j])


def test_ssq_cwt_long_vs_oracle(S, orc, case):
    """The fused form at the same lengths: the column-tile kernel over classes of up to 2^20 points
    (four-step 1024 x 1024), with `dWx` and lean, against the float32 oracle; `Tx` against the
    oracle's reassignment of the device's own `Wx`, `dWx`."""
    check_ssq_cwt_long(S, orc, case)


def test_ssq_cwt_long_tile_modes(S, orc, tile_mode):
    """The shortest of the lengths under both tile kernels (float64 tile / ordered)."""
    check_ssq_cwt_long(S, orc, make_case(orc, NS[0]))


def test_long_batch_equals_single(S, monkeypatch, N=600001):
    """Two signals in one call, both Nyquist rows on the exact passes (1024 x 1024): `blockIdx.z` in
    both passes and each signal's own slab of the intermediate `Z`."""
    from ssqueezepy_amd import _cwt
    from ssqueezepy_amd.wavelets import Wavelet
    from ssqueezepy_amd.scales import process_scales
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    sc = np.asarray(process_scales('log', N, Wavelet(('gmw', {'dtype': 'float32'})), nv=4),
                    dtype='float32').reshape(-1)[::2][:N_ROWS[N]]
    x = two_chirps(N, seed=N)
    xb = np.stack([x, x[::-1].copy()])
    monkeypatch.setenv('SSQ_DEBUG_CWT_NYQ_EXT', '0')
    _cwt.clear_plan_cache()
    try:
        Wb, _, dWb = S.cwt(xb, wav, scales=sc, derivative=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert 'fourstep' in plan.algo and plan.block_rows == len(sc) - 2 and plan.extended_rows == 0
        for b in range(2):
            W1, _, dW1 = S.cwt(xb[b], wav, scales=sc, derivative=True, astensor=False)
            assert np.array_equal(Wb[b], W1) and np.array_equal(dWb[b], dW1), b
        assert not np.array_equal(Wb[0, :2], Wb[1, :2])
    finally:
        _cwt.clear_plan_cache()
