# -*- coding: utf-8 -*-
"""Transform-level parity on the MI355X: cwt / ssq_cwt / stft / ssq_stft through
the public API (-> C ABI) against (1) fixtures produced by the reference itself and
(2) the CPU oracle pipeline on the same inputs.

Tolerances (BASELINE.json north_star): float32 <= 1e-5, float64 <= 1e-12, relative
to the array's max magnitude, on Wx/dWx/Sx/dSx. `Tx` is discontinuous in its inputs
(a point near a bin edge moves whole bins under 1-ulp input changes: SURVEY.md
section 7 hard part 2; the reference's own GPU-vs-CPU tolerance is atol 6e-3 / 1e-2,
tests/fft_test.py:449,587), so it is checked three ways: exactly, by feeding the
device's own Wx/dWx to the oracle reassignment; through its assignment-invariant
column sums; and elementwise with the reference's tolerance.
"""
import numpy as np
import pytest
from conftest import golden, two_chirps, assert_tx_vs_oracle, assert_tx_repeat, report_measured
from pipeline import oracle_ssq_cwt, oracle_ssq_stft, oracle_cwt_rows_float64, row_errors, GRIDNAME

pytestmark = pytest.mark.gpu
NUMBA = 0
RTOL = {'float32': 1e-5, 'float64': 1e-12}


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def check_Tx(orc, Tx, Wx, dWx, r, dtype, flipud=True, Sfs=None, grid=None):
    """Tx vs the oracle reassignment of the device's own (Wx, dWx): exact."""
    grid = GRIDNAME[r['grid']] if grid is None else grid
    ref = orc.ssqueeze(Wx, dWx, grid, r['params'], r['const'], r['gamma'], flipud,
                       Sfs=Sfs, typing=NUMBA)
    # (bit for bit, except for a Tx the unordered tile kernel produced: conftest.assert_tx_vs_oracle)
    from conftest import assert_tx_vs_oracle
    assert_tx_vs_oracle(Tx, ref, tiles=None if Sfs is None else False)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_ssq_cwt_vs_reference(S, orc, dtype):
    g = golden('cwt_' + dtype)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    cases = [(256, 'log', 16), (256, 'log-piecewise', 16), (1000, 'log', 8)]
    if dtype == 'float32':
        cases.append((256, 'linear', None))
    for N, st, nv in cases:
        x = g[f'x/{N}']
        Tx, Wx, ssq_freqs, scales, dWx = S.ssq_cwt(x, wav, scales=st, nv=nv,
                                                   get_dWx=True)
        Tx, Wx, dWx = _np(Tx), _np(Wx), _np(dWx)
        pre = f'{N}/{st}'
        assert Wx.dtype == g[f'Wx/{pre}'].dtype and Tx.dtype == Wx.dtype
        assert scales.dtype == np.dtype(dtype) and ssq_freqs.dtype == np.float64
        assert np.array_equal(scales, g[f'scales/{pre}'])
        assert np.array_equal(ssq_freqs, g[f'ssq_freqs/{pre}'])
        assert relmax(Wx, g[f'Wx/{pre}']) <= RTOL[dtype], (pre, relmax(Wx, g[f'Wx/{pre}']))
        if f'dWx/{pre}' in g:
            assert relmax(dWx, g[f'dWx/{pre}']) <= RTOL[dtype]
        # Tx: (1) exact given the device's own Wx, dWx
        r = oracle_ssq_cwt(orc, x, dtype, scales=st, nv=nv)
        check_Tx(orc, Tx, Wx, dWx, r, dtype)
        # (2) assignment-invariant column sums vs the reference
        ref = g[f'Tx/{pre}']
        assert np.abs(Tx.sum(0) - ref.sum(0)).max() <= 10 * RTOL[dtype] * np.abs(ref.sum(0)).max()
        # (3) elementwise at the reference's own GPU tolerance (fft_test.py:449)
        if dtype == 'float64':
            assert (np.abs(Tx - ref) > 1e-8).mean() < 2e-3
        else:
            assert np.abs(Tx - ref).mean() < 4e-5


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_ssq_cwt_options(S, orc, dtype):
    g = golden('cwt_' + dtype)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    x = g['x/256']
    # get_w: two-step form
    Tx, Wx, sf, sc, w, dWx = S.ssq_cwt(x, wav, scales='log', nv=16, get_w=True,
                                       get_dWx=True)
    Tx, Wx, w, dWx = map(_np, (Tx, Wx, w, dWx))
    wref = g['w/256/log']
    fin = np.isfinite(wref)
    assert np.array_equal(np.isfinite(w), fin)
    # w = Im(dWx/Wx)/2pi is ill-conditioned where |Wx| is tiny: compare where the
    # transform has energy ("dWx/w where |Wx| >> gamma")
    strong = fin & (np.abs(g['Wx/256/log']) > 1e-2 * np.abs(g['Wx/256/log']).max())
    assert strong.mean() > 0.2
    assert np.allclose(w[strong], wref[strong],
                       rtol=1e-3 if dtype == 'float32' else 1e-9)
    r = oracle_ssq_cwt(orc, x, dtype, scales='log', nv=16)
    assert np.array_equal(w, orc.phase_cwt(Wx, dWx, r['gamma'], typing=NUMBA))
    ref = orc.indexed_sum(Wx, w, 'log', r['params'], r['const'], True, typing=NUMBA)
    assert (Tx != ref).mean() < 1e-3 and np.abs(Tx - ref).mean() < 1e-8
    # flipud=False
    Tx2, Wx2, *_ = S.ssq_cwt(x, wav, scales='log', nv=16, flipud=False, astensor=False)
    Txf, *_ = S.ssq_cwt(x, wav, scales='log', nv=16, astensor=False)
    assert_tx_repeat(Tx2, Txf[::-1])
    # fs != 1 (derivative scaling by 1/dt)
    x = g['x/300']
    Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=8, fs=400.,
                                    get_dWx=True, astensor=False)
    assert relmax(Wx, g['Wx/300/fs400']) <= RTOL[dtype]
    assert relmax(dWx, g['dWx/300/fs400']) <= RTOL[dtype]
    assert np.array_equal(sf, g['ssq_freqs/300/fs400'])
    r = oracle_ssq_cwt(orc, x, dtype, scales='log', nv=8, fs=400.)
    check_Tx(orc, Tx, Wx, dWx, r, dtype)
    # batched == looped (reference: tests/fft_test.py:559-596), and vs fixtures
    xb = g['x/batch200']
    Txb, Wxb, *_ = S.ssq_cwt(xb, wav, scales='log', nv=8, astensor=False)
    assert Txb.shape == g['Tx/batch200'].shape
    for b in range(len(xb)):
        Tx1, Wx1, *_ = S.ssq_cwt(xb[b], wav, scales='log', nv=8, astensor=False)
        assert np.array_equal(Wxb[b], Wx1)
        assert_tx_repeat(Txb[b], Tx1)
        assert relmax(Wxb[b], g['Wx/batch200'][b]) <= RTOL[dtype]


def test_cwt_paddings_families_and_rpadded(S, orc):
    g = golden('cwt_float32')
    x = g['x/300']
    for pt in ('zero', 'symmetric', 'replicate', 'wrap', None):
        Wx, sc = S.cwt(x, 'gmw', scales='log', nv=8, padtype=pt, astensor=False)
        ref = g['Wx/300/pad_' + (pt or 'none')]
        assert relmax(Wx, ref) <= 1e-5, (pt, relmax(Wx, ref))
    Wxp, sc, dWxp = S.cwt(x, 'gmw', scales='log', nv=8, rpadded=True,
                          derivative=True, astensor=False)
    Wx, sc, dWx = S.cwt(x, 'gmw', scales='log', nv=8, derivative=True,
                        astensor=False)
    n1 = (512 - 300) - (512 - 300) // 2
    assert Wxp.shape[-1] == 512
    assert np.array_equal(Wxp[:, n1:n1 + 300], Wx)
    assert np.array_equal(dWxp[:, n1:n1 + 300], dWx)
    g = golden('cwt_families')
    x = g['x']
    for name in ('morlet', 'bump', 'cmhat', 'hhhat'):
        Tx, Wx, sf, sc = S.ssq_cwt(x, name, scales='log', nv=8, astensor=False)
        assert relmax(Wx, g[f'Wx/{name}']) <= 1e-5, name
        assert np.array_equal(sf, g[f'ssq_freqs/{name}'])
        ref = g[f'Tx/{name}']
        assert np.abs(Tx.sum(0) - ref.sum(0)).max() <= 1e-4 * np.abs(ref.sum(0)).max()
    Wx, sc = S.cwt(x, 'morlet', scales='log', nv=8, l1_norm=False, astensor=False)
    assert relmax(Wx, g['Wx/morlet_l2']) <= 1e-5


def test_cwt_input_handling(S):
    import torch
    x = two_chirps(500, seed=4)
    xbad = x.copy()
    xbad[10] = np.nan
    xbad[20] = np.inf
    Wx, _ = S.cwt(xbad, 'gmw', scales='log', nv=8, astensor=False)
    assert xbad[10] == 0 and xbad[20] == 0         # zeroed in the caller's array
    xz = x.copy(); xz[10] = 0; xz[20] = 0
    Wz, _ = S.cwt(xz, 'gmw', scales='log', nv=8, astensor=False)
    assert np.array_equal(Wx, Wz)
    Wt, _ = S.cwt(torch.as_tensor(xz), 'gmw', scales='log', nv=8)
    assert isinstance(Wt, torch.Tensor) and Wt.is_cuda and Wt.dtype == torch.complex64
    assert np.array_equal(_np(Wt), Wz)
    with pytest.raises(ValueError):
        S.cwt(np.zeros((2, 2, 8)), 'gmw')
    with pytest.raises(TypeError):
        S.cwt([1., 2., 3.], 'gmw')
    with pytest.raises(NotImplementedError):
        S.ssq_cwt(np.zeros((2, 64)), 'gmw', get_w=True)
    with pytest.raises(ValueError):
        S.ssq_cwt(x, 'gmw', difftype='numeric', get_w=True)
    # linearity of the CWT
    y = two_chirps(500, seed=5)
    Wy, _ = S.cwt(y, 'gmw', scales='log', nv=8, astensor=False)
    Wxy, _ = S.cwt(2 * xz - 3 * y, 'gmw', scales='log', nv=8, astensor=False)
    assert relmax(Wxy, 2 * Wz - 3 * Wy) < 2e-6


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_ssq_stft_vs_reference(S, orc, dtype):
    g = golden('stft_' + dtype)
    for N, n_fft, hop in ((256, 64, 1), (1000, 128, 32), (2000, 256, 64),
                          (777, 100, 7)):
        pre = f'{N}/{n_fft}/{hop}'
        x = g['x/' + pre]
        Tx, Sx, sf, Sfs, dSx = S.ssq_stft(x, n_fft=n_fft, hop_len=hop, dtype=dtype,
                                          get_dWx=True, astensor=False)
        assert Sx.shape == g['Sx/' + pre].shape and Sx.dtype == g['Sx/' + pre].dtype
        assert relmax(Sx, g['Sx/' + pre]) <= RTOL[dtype], (pre, relmax(Sx, g['Sx/' + pre]))
        assert relmax(dSx, g['dSx/' + pre]) <= RTOL[dtype]
        assert np.array_equal(Sfs, g['Sfs/' + pre]) and np.array_equal(sf, g['ssq_freqs/' + pre])
        r = oracle_ssq_stft(orc, x, dtype, n_fft=n_fft, hop_len=hop)
        from ssqueezepy_amd.ssqueezing import ssq_grid_params
        _, p = ssq_grid_params(Sfs, False)
        ref = orc.ssqueeze(Sx, dSx, 'linear', p, Sfs[1] - Sfs[0], r['gamma'], False,
                           Sfs=Sfs, typing=NUMBA)
        assert np.array_equal(Tx, ref)
        gref = g['Tx/' + pre]
        assert np.abs(Tx.sum(0) - gref.sum(0)).max() <= 10 * RTOL[dtype] * np.abs(gref.sum(0)).max()
    x = g['x/600']
    Sx, dSx = S.stft(x, n_fft=128, hop_len=16, modulated=False, derivative=True,
                     dtype=dtype, fs=10., astensor=False)
    assert relmax(Sx, g['Sx/600/nomod']) <= RTOL[dtype]
    assert relmax(dSx, g['dSx/600/nomod']) <= RTOL[dtype]
    out = S.ssq_stft(x, n_fft=128, hop_len=16, dtype=dtype, get_w=True, fs=10.,
                     astensor=False)
    wref = g['w/600/getw']
    fin = np.isfinite(wref)
    assert np.array_equal(np.isfinite(out[4]), fin)
    Sref = np.abs(oracle_ssq_stft(orc, x, dtype, n_fft=128, hop_len=16, fs=10.,
                                  ssq=False)['Sx'])
    strong = fin & (Sref > 1e-2 * Sref.max())
    assert strong.mean() > 0.05
    assert np.allclose(out[4][strong], wref[strong],
                       rtol=1e-3 if dtype == 'float32' else 1e-9,
                       atol=1e-4 if dtype == 'float32' else 1e-11)
    Sx = S.stft(x, 'hann', n_fft=128, win_len=100, hop_len=16, dtype=dtype,
                astensor=False)
    assert relmax(Sx, g['Sx/600/hann100']) <= RTOL[dtype]
    xb = g['x/batch400']
    Txb, Sxb, *_ = S.ssq_stft(xb, n_fft=64, hop_len=8, dtype=dtype, astensor=False)
    assert relmax(Sxb, g['Sx/batch400']) <= RTOL[dtype]
    for b in range(len(xb)):
        T1, S1, *_ = S.ssq_stft(xb[b], n_fft=64, hop_len=8, dtype=dtype, astensor=False)
        assert_tx_repeat(Txb[b], T1)
        assert np.array_equal(Sxb[b], S1)


def test_ssqueeze_standalone(S, orc):
    """`ssqueeze` on a device CWT == the fused ssq_cwt (reference:
    tests/fft_test.py:351-377, fused == two-step)."""
    x = two_chirps(512, seed=8)
    wav = S.Wavelet()
    Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=16, get_dWx=True)
    Tx2, sf2 = S.ssqueeze(Wx, None, 'log', sc, wavelet=wav, maprange='peak',
                          gamma=10 * S.EPS32, flipud=True, dWx=dWx)
    assert_tx_vs_oracle(_np(Tx), _np(Tx2))       # (fused: float64 sums; two-step: the ordered sums)
    assert np.array_equal(sf, sf2)
    w = S.phase_cwt(Wx, dWx, gamma=10 * S.EPS32)
    Tx3, _ = S.ssqueeze(Wx, w, 'log', sc, wavelet=wav, maprange='peak', flipud=True)
    assert np.abs(_np(Tx3) - _np(Tx)).mean() < 4e-5     # fft_test.py:470


def test_full_size_properties(S):
    """BASELINE config 2 (N=160 000, 300 scales, float32) at full size, through
    size-independent properties: the assignment-invariant checksum
    sum_k Tx[k, j] == sum_i Wx[i, j] * const_i, linearity of Wx, and
    batched == single."""
    import torch
    N, na = 160000, 300
    wav = S.Wavelet()
    scales = S.process_scales('log', N, wav, nv=32)[:na]
    x = two_chirps(N, seed=0)
    Tx, Wx, sf, sc = S.ssq_cwt(x, wav, scales=scales)
    assert Tx.shape == (na, N) and Wx.shape == (na, N)
    const = np.log(2) / 32
    lhs = Tx.sum(0)
    rhs = (Wx * const).sum(0)
    err = (lhs - rhs).abs().max().item() / rhs.abs().max().item()
    assert err < 2e-5, err
    y = two_chirps(N, seed=1)
    Wy, _ = S.cwt(y, wav, scales=scales)
    Wxy, _ = S.cwt(0.5 * x + 2 * y, wav, scales=scales)
    lin = (Wxy - (0.5 * Wx + 2 * Wy)).abs().max().item() / Wxy.abs().max().item()
    assert lin < 5e-6, lin
    xb = np.stack([x, y])
    Txb, Wxb, *_ = S.ssq_cwt(xb, wav, scales=scales)
    Ty, Wy2, *_ = S.ssq_cwt(y, wav, scales=scales)
    assert torch.equal(Wxb[0], Wx) and torch.equal(Wxb[1], Wy2)
    assert_tx_repeat(_np(Txb[0]), _np(Tx))
    assert_tx_repeat(_np(Txb[1]), _np(Ty))
    # `cwt` (block kernels for every row) and the fused `ssq_cwt` (column tiles: most rows
    # interpolated from decimated samples) evaluate the same rows in two ways
    assert (Wy2 - Wy).abs().max().item() <= 6e-6 * Wy.abs().max().item()


def test_full_size_bin_map_exact(S, orc):
    """BASELINE config 2 at full size: the oracle reassigns this engine's own (Wx, dWx) and `Tx`
    is compared with the result. With `SSQ_TILE_ORDER=ordered` (the ticketed kernel; the `tile_mode`
    fixture and test_gpu_00_configs run it) equal `Tx`, cell for cell, means every one of the 48 M
    indices and the summation order agree. In the DEFAULT mode (float64 tile, unordered adds) the
    comparison is to 1e-6 of the largest cell: it pins the sums and every bin whose point weighs more
    than that -- not the indices of points below it. Those are pinned as integers by
    test_gpu_00_configs.py::test_config2_bin_indices_are_the_oracles_integers (a bin dump of the same
    kernel against the oracle's map, `array_equal`); this test keeps the lean / full build comparison."""
    N, na = 160000, 300
    wav = S.Wavelet()
    scales = S.process_scales('log', N, wav, nv=32)[:na]
    x = two_chirps(N, seed=3)
    Tx, Wx, sf, sc = S.ssq_cwt(x, wav, scales=scales, astensor=False)          # lean kernels
    Tx2, Wx2, _, _, dWx = S.ssq_cwt(x, wav, scales=scales, get_dWx=True, astensor=False)
    assert np.array_equal(Wx, Wx2)
    assert_tx_repeat(Tx, Tx2)
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    kind, p = ssq_grid_params(sf[::-1], True)      # ssq_cwt returns the flipped (descending) grid
    st = {0: 'log', 1: 'log-piecewise'}[kind]
    gamma = 10 * np.finfo(np.float32).eps
    ref = orc.ssqueeze(Wx, dWx, st, p, np.log(2) / 32, gamma, True, typing=0, parallel=True)
    assert_tx_vs_oracle(Tx2, ref)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('N,nv,wavelet', [(20011, 8, 'gmw'), (70001, 8, 'morlet'), (70001, 4, 'morlet')])
def test_nyquist_rows_continued_vs_exact_paths(S, orc, N, nv, wavelet, dtype, monkeypatch):
    """Rows cut by the Nyquist bin: continued past it and run by the block kernels over the
    analytic signal (default; _blocks.extend_past_nyquist) -- and, with SSQ_DEBUG_CWT_NYQ_EXT=0, on the
    exact paths they had before (float32: four-step kernels, float64: banded multiply + rocFFT).
    Both against the oracle of the reference's full-length algorithm, and against each other."""
    from ssqueezepy_amd import _cwt
    tol = 1e-5 if dtype == 'float32' else 1e-12
    x = two_chirps(N, seed=N)
    wav = S.Wavelet((wavelet, {'dtype': dtype}))
    r = oracle_ssq_cwt(orc, x, dtype, wavelet=wavelet, scales='log', nv=nv, typing=1)
    out = {}
    for ext in ('1', '0'):
        monkeypatch.setenv('SSQ_DEBUG_CWT_NYQ_EXT', ext)
        _cwt.clear_plan_cache()
        Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        if ext == '1':
            # every cut row continued -- except the first row of the coarse Morlet bank (nv = 4), whose
            # peak lies far past Nyquist: the gain limit (_blocks.NYQ_EXT_GAIN) leaves it on the exact path
            refused = 1 if (wavelet, nv) == ('morlet', 4) else 0
            assert plan.extended_rows >= 3 and plan.block_rows == len(sc) - refused, (plan.algo, plan.extended_rows)
            assert (('fourstep' in plan.algo) or ('rocfft' in plan.algo)) == (refused > 0), plan.algo
        else:
            assert plan.extended_rows == 0 and plan.block_rows < len(sc)
            assert ('fourstep' if dtype == 'float32' else 'rocfft') in plan.algo, plan.algo
        eW, eD = relmax(Wx, r['Wx']), relmax(dWx, r['dWx'])
        assert eW <= tol and eD <= tol, (ext, eW, eD)
        check_Tx(orc, Tx, Wx, dWx, r, dtype)
        if dtype == 'float32' and ext == '0':
            # the rows on the four-step kernels, each against its OWN size (the first cut row is a few 1e-3 of
            # the array's maximum: `relmax` cannot see it): a float64 statement from the float32 bank, the
            # float32 oracle's row error as the yardstick (tests/test_gpu_long_signals.py)
            rows = np.arange(len(sc) - plan.block_rows)
            W64, D64 = oracle_cwt_rows_float64(orc, x, sc, rows, wavelet=wavelet)
            for name, dev, ref32, ref64 in (('Wx', Wx, r['Wx'], W64), ('dWx', dWx, r['dWx'], D64)):
                e_dev, e_orc = row_errors(dev[rows], ref64), row_errors(ref32[rows], ref64)
                report_measured('nyquist_rows_exact_per_row', N=N, wavelet=wavelet, nv=nv, what=name,
                                rows=len(rows), dev=e_dev.max(), orc=e_orc.max(), ratio=(e_dev / e_orc).max())
                assert (e_dev <= 2 * e_orc).all(), (name, e_dev, e_orc)
        out[ext] = (Wx, plan.extended_rows)
    n_cut = out['1'][1] + (1 if (wavelet, nv) == ('morlet', 4) else 0)
    assert relmax(out['1'][0][:n_cut], out['0'][0][:n_cut]) <= tol
    _cwt.clear_plan_cache()


@pytest.mark.parametrize('N,padtype', [(3000, 'reflect'), (10000, 'reflect'), (10000, 'zero'), (6000, 'symmetric'), (20000, 'reflect')])
def test_short_signal_prestage_and_spectra_in_one_launch(S, orc, N, padtype, monkeypatch):
    """Short float32 signals (M = 8192 / 16384; BASELINE config 1's shape): `small_prestage_kernel` (pad + forward
    transform + analytic signal, one workgroup per signal) and `block_spectra_multi_kernel` (the P = 4096 / 8192 /
    16384 classes' spectra in one launch) against the routes they replace (pad kernel + rocFFT + four-step analytic
    signal + gather + rocFFT: SSQ_DEBUG_BLOCK_SPECTRA=rocfft), against the oracle of the reference's full-length
    algorithm, and a batch (one workgroup per signal) against its signals one at a time."""
    from ssqueezepy_amd import _cwt
    nv = 8
    x = two_chirps(N, seed=N).astype(np.float32)
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    out = {}
    for mode in ('', 'rocfft'):
        if mode:
            monkeypatch.setenv('SSQ_DEBUG_BLOCK_SPECTRA', mode)
        else:
            monkeypatch.delenv('SSQ_DEBUG_BLOCK_SPECTRA', raising=False)
        _cwt.clear_plan_cache()
        Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=nv, padtype=padtype, get_dWx=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.algo.startswith('blockzoom')
        assert plan.block_plan['classes'][:, 0].max() >= 8192     # (a class the P = 4096-only kernel does not serve)
        out[mode] = (Wx, dWx, Tx)
    monkeypatch.delenv('SSQ_DEBUG_BLOCK_SPECTRA', raising=False)
    _cwt.clear_plan_cache()
    eW, eD = relmax(out[''][0], out['rocfft'][0]), relmax(out[''][1], out['rocfft'][1])
    assert eW <= 2e-6 and eD <= 2e-6, (eW, eD)
    # a plain cwt (Wx alone: the block kernels' instantiation without the derivative) gives the Wx of a cwt with its
    # derivative, bit for bit
    Wc = S.cwt(x, wav, scales='log', nv=nv, padtype=padtype, astensor=False)[0]
    Wd, _, dWd = S.cwt(x, wav, scales='log', nv=nv, padtype=padtype, derivative=True, astensor=False)
    assert np.array_equal(Wc, Wd)
    assert relmax(Wd, out[''][0]) <= 5e-6 and relmax(dWd, out[''][1]) <= 5e-6      # (ssq_cwt's rows come from the tile kernel)
    if padtype == 'reflect':
        r = oracle_ssq_cwt(orc, x, 'float32', scales='log', nv=nv, typing=1)
        eW, eD = relmax(out[''][0], r['Wx']), relmax(out[''][1], r['dWx'])
        assert eW <= 1e-5 and eD <= 1e-5, (eW, eD)
        check_Tx(orc, out[''][2], out[''][0], out[''][1], r, 'float32')
    xb = np.stack([x, x[::-1].copy(), 0.5 * x])
    Wxb = S.cwt(xb, wav, scales='log', nv=nv, padtype=padtype, astensor=False)[0]
    for i in range(3):
        Wi = S.cwt(xb[i], wav, scales='log', nv=nv, padtype=padtype, astensor=False)[0]
        assert np.array_equal(Wxb[i], Wi)
    _cwt.clear_plan_cache()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('N,nv', [(6000, 16), (20000, 8), (40000, 4)])
def test_block_fast_path_vs_oracle(S, orc, N, nv, dtype):
    """The block ("overlap-save zoom") fast path -- active once the padded length
    reaches 4096, in float32 and float64 -- against the CPU oracle of the reference's
    full-length algorithm (1e-5 / 1e-12), and against this engine's own exact (rocFFT)
    path."""
    import os
    from ssqueezepy_amd import _cwt
    tol = 1e-5 if dtype == 'float32' else 1e-12
    x = two_chirps(N, seed=N)
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    _cwt.clear_plan_cache()
    Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True,
                                    astensor=False)
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    assert plan.algo.startswith('blockzoom') and plan.block_rows > 0.8 * len(sc)
    r = oracle_ssq_cwt(orc, x, dtype, scales='log', nv=nv, typing=1)
    assert np.array_equal(sf, r['ssq_freqs']) and np.array_equal(sc, r['scales'])
    eW, eD = relmax(Wx, r['Wx']), relmax(dWx, r['dWx'])
    assert eW <= tol and eD <= tol, (eW, eD)
    check_Tx(orc, Tx, Wx, dWx, r, dtype)
    assert np.abs(Tx.sum(0) - r['Tx'].sum(0)).max() <= 10 * tol * np.abs(r['Tx'].sum(0)).max()
    # exact path of this engine on the same input
    os.environ['SSQ_DEBUG_CWT_ALGO'] = 'generic'
    try:
        _cwt.clear_plan_cache()
        Tx2, Wx2, _, _, dWx2 = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True,
                                         astensor=False)
        plan2 = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan2.algo == 'rocfft'
    finally:
        del os.environ['SSQ_DEBUG_CWT_ALGO']
        _cwt.clear_plan_cache()
    assert relmax(Wx2, r['Wx']) <= tol and relmax(dWx2, r['dWx']) <= tol
    assert relmax(Wx, Wx2) <= tol
    # get_w / batched through the block path
    out = S.ssq_cwt(x, wav, scales='log', nv=nv, get_w=True, get_dWx=True, astensor=False)
    assert np.array_equal(out[4], orc.phase_cwt(out[1], out[5], r['gamma'], typing=0))
    assert relmax(out[1], Wx) <= tol / 2      # two-step form: every row on the block kernels
    # a plain cwt runs the kernels' Wx-only instantiation (no derivative transform): the same Wx, bit for bit
    Wc = S.cwt(x, wav, scales='log', nv=nv, astensor=False)[0]
    Wd = S.cwt(x, wav, scales='log', nv=nv, derivative=True, astensor=False)[0]
    assert np.array_equal(Wc, Wd) and relmax(Wc, r['Wx']) <= tol
    xb = np.stack([x, x[::-1].copy()])
    Txb, Wxb, *_ = S.ssq_cwt(xb, wav, scales='log', nv=nv, astensor=False)
    assert np.array_equal(Wxb[0], Wx)
    assert_tx_repeat(Txb[0], Tx)
    T1, W1, *_ = S.ssq_cwt(xb[1], wav, scales='log', nv=nv, astensor=False)
    assert np.array_equal(Wxb[1], W1)
    assert_tx_repeat(Txb[1], T1)


def test_ssqueeze_squeezing_modes_and_stft_config3(S, orc):
    """`ssqueeze` with squeezing='lebesgue' / 'abs' (ssqueezing.py:197-202), and
    BASELINE config 3 (ssq_stft N=160 000, n_fft=1024, hop=256) at full size against the
    oracle reassignment of the device's own Sx, dSx."""
    import torch
    x = two_chirps(1024, seed=2)
    wav = S.Wavelet()
    Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=8, get_dWx=True)
    r = oracle_ssq_cwt(orc, x, 'float32', scales='log', nv=8)
    Wn, dWn = _np(Wx), _np(dWx)
    for mode in ('lebesgue', 'abs'):
        T2, _ = S.ssqueeze(Wx, None, 'log', sc, wavelet=wav, maprange='peak',
                           gamma=r['gamma'], flipud=True, dWx=dWx, squeezing=mode)
        # |Wx| as the device forms it (torch.abs and hypotf may differ in the last bit)
        Wm = ((np.ones_like(Wn) / len(Wn)) if mode == 'lebesgue' else
              _np(torch.abs(Wx)).astype(Wn.dtype))
        ref = orc.ssqueeze(Wm, dWn, 'log', r['params'], r['const'], r['gamma'], True, typing=NUMBA)
        assert np.array_equal(_np(T2), ref), mode
        # the same mode through ssq_cwt itself (returned Wx stays the transform)
        T3, W3, *_ = S.ssq_cwt(x, wav, scales='log', nv=8, squeezing=mode)
        assert torch.equal(W3, Wx), mode
        assert_tx_vs_oracle(_np(T3), _np(T2), what=mode)
    T4, *_ = S.ssq_cwt(x, wav, scales='log', nv=8, squeezing=lambda W: 2 * W)
    ref = orc.ssqueeze(2 * Wn, dWn, 'log', r['params'], r['const'], r['gamma'], True, typing=NUMBA)
    assert_tx_vs_oracle(_np(T4), ref)
    # config 3
    N = 160000
    x = two_chirps(N, seed=3)
    Tx, Sx, sf, Sfs, dSx = S.ssq_stft(x, n_fft=1024, hop_len=256, dtype='float32',
                                      get_dWx=True, astensor=False)
    assert Sx.shape == (513, 625)
    ro = oracle_ssq_stft(orc, x, 'float32', n_fft=1024, hop_len=256)
    assert relmax(Sx, ro['Sx']) <= 1e-5 and relmax(dSx, ro['dSx']) <= 1e-5
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    _, p = ssq_grid_params(Sfs, False)
    ref = orc.ssqueeze(Sx, dSx, 'linear', p, Sfs[1] - Sfs[0], ro['gamma'], False, Sfs=Sfs,
                       typing=NUMBA)
    assert np.array_equal(Tx, ref)
    Ta, Sa, *_ = S.ssq_stft(x, n_fft=1024, hop_len=256, dtype='float32', squeezing='abs',
                            astensor=False)
    ref = orc.ssqueeze(np.abs(Sx).astype(Sx.dtype), dSx, 'linear', p, Sfs[1] - Sfs[0],
                       ro['gamma'], False, Sfs=Sfs, typing=NUMBA)
    assert np.array_equal(Sa, Sx)
    assert (np.abs(Ta - ref) > 1e-6 * np.abs(ref).max()).mean() < 1e-4   # |.| last-bit ties


def test_float64_long_signal_properties(S):
    """BASELINE config 5 shape (float64, long signal) at reduced length: float64
    column-sum identity to 1e-12 and linearity."""
    import torch
    N, na = 131072, 128
    wav = S.Wavelet(('gmw', {'dtype': 'float64'}))
    scales = S.process_scales('log', N, wav, nv=16)[:na]
    x = two_chirps(N, seed=11)
    Tx, Wx, sf, sc = S.ssq_cwt(x, wav, scales=scales)
    assert Tx.dtype == torch.complex128 and sc.dtype == np.float64
    const = np.log(2) / 16
    lhs, rhs = Tx.sum(0), (Wx * const).sum(0)
    assert ((lhs - rhs).abs().max() / rhs.abs().max()).item() < 1e-12
    y = two_chirps(N, seed=12)
    Wy, _ = S.cwt(y, wav, scales=scales)
    Wxy, _ = S.cwt(x - 2 * y, wav, scales=scales)
    assert ((Wxy - (Wx - 2 * Wy)).abs().max() / Wxy.abs().max()).item() < 1e-13


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_higher_order_gmw_vs_reference(S, orc, dtype):
    """cwt / ssq_cwt with higher-order generalized Morse wavelets (order > 0, tuples with
    averaging) against the reference's outputs (tests/golden/hiorder.npz; wavelet samples
    are checked value-exact in test_design_vs_golden.py)."""
    g = golden('hiorder')
    tol = 1e-5 if dtype == 'float32' else 1e-11
    x = g[f'x/{dtype}']
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    Wx, sc, dWx = S.cwt(x, wav, scales='log', nv=8, order=1, derivative=True, astensor=False)
    assert np.array_equal(np.asarray(sc).reshape(-1), g[f'sc/{dtype}'].reshape(-1))
    assert relmax(Wx, g[f'Wx1/{dtype}']) <= tol and relmax(dWx, g[f'dWx1/{dtype}']) <= tol
    Wa, _ = S.cwt(x, wav, scales='log', nv=8, order=(0, 2), average=True, astensor=False)
    assert relmax(Wa, g[f'Wx02/{dtype}']) <= tol
    Wl, _ = S.cwt(x, wav, scales='log', nv=8, order=(0, 2), average=False, astensor=False)
    assert isinstance(Wl, list) and len(Wl) == 2
    assert relmax(0.5 * (Wl[0] + Wl[1]), g[f'Wx02/{dtype}']) <= tol
    for order, key in ((2, '2'), ((0, 1, 2), '012')):
        Tx, Wx, sf, sc, dWx = S.ssq_cwt(x, wav, scales='log', nv=8, order=order,
                                        get_dWx=True, astensor=False)
        assert np.array_equal(sf, g[f'sf/{dtype}'])
        assert relmax(Wx, g[f'WxT{key}/{dtype}']) <= tol
        # reassignment: exact w.r.t. the oracle on the device's own (Wx, dWx); against the
        # reference's Tx through the assignment-invariant column sums
        r = oracle_ssq_cwt(orc, x, dtype, scales='log', nv=8)
        check_Tx(orc, Tx, Wx, dWx, r, dtype)
        ref = g[f'Tx{key}/{dtype}']
        assert np.abs(Tx.sum(0) - ref.sum(0)).max() <= 20 * tol * np.abs(ref.sum(0)).max()
    with pytest.raises(ValueError):
        S.cwt(x, 'morlet', order=1)


@pytest.mark.parametrize('dtype,padtype,l1_norm', [('float64', 'reflect', True), ('float64', 'zero', False),
                                                  ('float64', 'wrap', True), ('float32', 'symmetric', True)])
def test_cwt_is_differentiable(S, dtype, padtype, l1_norm):
    """`cwt` of a tensor that requires grad (examples/reconstruction.py:1-70: gradient-based
    scalogram inversion): the custom backward (adjoint of the plan) against torch.autograd
    through a plain torch.fft statement of the same transform."""
    import torch
    from ssqueezepy_amd import _cwt
    dev = 'cpu' if __import__('os').environ.get('SSQ_EMULATE') == '1' else 'cuda'
    N, B = 300, 2
    rng = np.random.default_rng(3)
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    wav = S.Wavelet(('gmw' if l1_norm else 'morlet', {'dtype': dtype}))
    x0 = torch.as_tensor(np.stack([two_chirps(N, 1), two_chirps(N, 2)]), dtype=tdt, device=dev)
    wgt = torch.as_tensor(rng.random((B, 1, N)) + 0.5, dtype=tdt, device=dev)
    _cwt.clear_plan_cache()

    x = x0.clone().requires_grad_(True)
    Wx, scales = S.cwt(x, wav, nv=8, padtype=padtype, l1_norm=l1_norm)
    assert Wx.requires_grad
    loss = (torch.abs(Wx)**2 * wgt).sum() + (Wx.real * wgt).sum()
    loss.backward()
    plan = next(iter(_cwt._PLAN_CACHE.values()))

    # the same linear map with torch ops
    psih = plan.dense_bank(x0.device)
    src = plan.pad_sources(x0.device)
    xr = x0.clone().requires_grad_(True)
    xp = torch.where(src >= 0, xr[:, src.clamp(min=0)], torch.zeros((), dtype=tdt, device=dev))
    Wr = torch.fft.ifft(psih[None] * torch.fft.fft(xp, dim=-1)[:, None], dim=-1)
    Wr = Wr[..., plan.n1:plan.n1 + N]
    tol = 1e-5 if dtype == 'float32' else 1e-12
    assert relmax(_np(Wx.detach()), _np(Wr.detach())) <= tol
    lr = (torch.abs(Wr)**2 * wgt).sum() + (Wr.real * wgt).sum()
    lr.backward()
    assert relmax(_np(x.grad), _np(xr.grad)) <= 20 * tol
    # a 1-D signal, and no gradient bookkeeping when it is not asked for
    x1 = x0[0].clone().requires_grad_(True)
    W1, _ = S.cwt(x1, wav, nv=8, padtype=padtype, l1_norm=l1_norm)
    (torch.abs(W1)**2 * wgt[0]).sum().backward()
    xr1 = x0[0].clone().requires_grad_(True)
    xp1 = torch.where(src >= 0, xr1[src.clamp(min=0)], torch.zeros((), dtype=tdt, device=dev))
    Wr1 = torch.fft.ifft(psih * torch.fft.fft(xp1)[None], dim=-1)[:, plan.n1:plan.n1 + N]
    (torch.abs(Wr1)**2 * wgt[0]).sum().backward()
    assert relmax(_np(x1.grad), _np(xr1.grad)) <= 20 * tol
    with torch.no_grad():
        assert not S.cwt(x1, wav, nv=8, padtype=padtype, l1_norm=l1_norm)[0].requires_grad
    _cwt.clear_plan_cache()
