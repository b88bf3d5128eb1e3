# -*- coding: utf-8 -*-
"""The block rows' band staged once per workgroup in the transform buffer (csrc/ssq_cwt_blocks.hip: `BAND`) on the device
against the paired kernels with the band outside the buffer (`SSQ_DEBUG_BLOCK_BAND=0`, read when a plan is created):
every value is made by the same operations on the same operands in the same order, so `Wx`, `dWx` and every point's bin
are equal bit for bit, and `Tx` as two runs on the same data are. Shapes: those of tests/test_gpu_block_paired.py --
every transform length L' = 128 .. 2048, workgroups that own all columns of their block and workgroups that own some,
blocks of the analytic signal, classes P = 4096, 8192 and 16384 -- each in the full build (dWx stored) and the lean one
(the benchmarked kernel), and as a plain cwt with its derivative. The plans' row tables hold what the staging has to
get right: bands narrower than half their transform (zero slots), and for L' = 1024 and 2048 first bins off the
work-items' 256-element stride and bands that run past the transform's end."""
import numpy as np
import pytest
from conftest import two_chirps, assert_tx_repeat, tile_order

pytestmark = pytest.mark.gpu

SHAPES = ((1500, 8), (3000, 16), (6000, 16))


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def _fused(S, x, wav, nv):
    """ssq_cwt, lean and full build, with every point's bin dumped as the reassignment consumed it (the ordered tile
    kernel keeps no dump: its Tx is a fixed-order sum of the same terms, so Tx pins the bins there)."""
    import torch
    from ssqueezepy_amd import _cwt, algos
    _cwt.clear_plan_cache()
    S.ssq_cwt(x, wav, scales='log', nv=nv)                     # (creates the plan)
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    assert plan.algo.startswith('blockzoom') and plan.block_rows > 0.5 * plan.na, plan.algo
    N, nsig = x.shape[-1], (1 if x.ndim == 1 else len(x))
    dump = not (plan.tile_cols and tile_order() == 'ordered')
    kmap = torch.full((plan.max_batch * plan.na * N,), -2, dtype=torch.int16, device=algos.device())
    if dump:
        plan.set_bin_dump(kmap)
    try:
        Tl, Wl, *_ = S.ssq_cwt(x, wav, scales='log', nv=nv)
        k_lean = kmap.clone()
        kmap.fill_(-2)
        Tf, Wf, _, _, Df = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True)
        k_full = kmap.clone()
    finally:
        if dump:
            plan.set_bin_dump(None)
    if dump:
        assert not bool((k_full[:nsig * plan.na * N] == -2).any())             # every point written
    out = dict(algo=plan.algo, Wx_lean=Wl, Wx_full=Wf, dWx_full=Df, k_lean=k_lean, k_full=k_full,
               Tx_lean=Tl.cpu().numpy(), Tx_full=Tf.cpu().numpy(), tiles=bool(plan.tile_cols))
    _cwt.clear_plan_cache()
    return out


def _run(S, x, nv, monkeypatch, band):
    from ssqueezepy_amd import _cwt
    monkeypatch.delenv('SSQ_DEBUG_BLOCK_PAIRED', raising=False)
    if band is None:
        monkeypatch.delenv('SSQ_DEBUG_BLOCK_BAND', raising=False)
    else:
        monkeypatch.setenv('SSQ_DEBUG_BLOCK_BAND', band)
    wav = S.Wavelet()
    out = _fused(S, x, wav, nv)
    Wx, sc, dWx = S.cwt(x, wav, scales='log', nv=nv, derivative=True)
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    assert plan.algo.startswith('blockzoom'), plan.algo
    out.update(Wx=Wx, dWx=dWx, algo_cwt=plan.algo)
    _cwt.clear_plan_cache()
    return out


def _same(a, b, what):
    import torch
    assert a['algo'] == b['algo'] and a['algo_cwt'] == b['algo_cwt']
    for k in ('Wx', 'dWx', 'Wx_lean', 'Wx_full', 'dWx_full', 'k_lean', 'k_full'):
        assert torch.equal(a[k], b[k]), (what, k)
    for k in ('Tx_lean', 'Tx_full'):
        assert_tx_repeat(a[k], b[k], tiles=a['tiles'], what=(what, k))


def _check_rows(bp):
    """rows (cls, klo, KP, L', G, pb_off) of the block plan: every length has rows; a band narrower than L' / 2 (a row's
    L' is the shortest length that holds its band, so such a row sits in the shortest transform); the two long
    transforms have zero slots, first bins that are no multiple of 256 and bands with klo mod L' + KP > L'."""
    rows = bp['rows'][bp['rows'][:, 0] >= 0]
    assert sorted(set(rows[:, 3].tolist())) == [128, 256, 512, 1024, 2048]
    assert (rows[:, 2] <= rows[:, 3]).all() and (2 * rows[:, 2] < rows[:, 3]).any()
    for L in (1024, 2048):
        big = rows[rows[:, 3] == L]
        assert (big[:, 1] % 256 != 0).any() and (big[:, 2] < L).any() and ((big[:, 1] % L) + big[:, 2] > L).any(), L


@pytest.mark.parametrize('N,nv', SHAPES)
def test_band_in_the_transform_buffer_equals_band_outside(S, monkeypatch, N, nv):
    import torch
    from ssqueezepy_amd import _cwt
    seen = []
    real = _cwt.plan_blocks
    monkeypatch.setattr(_cwt, 'plan_blocks', lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    x = two_chirps(N, seed=5)
    on, off = (_run(S, x, nv, monkeypatch, b) for b in (None, '0'))
    _check_rows(seen[-1])
    _same(on, off, (N, nv))
    assert torch.equal(on['Wx_lean'], on['Wx_full'])           # (the two builds agree, as they did before)
    if on['tiles'] and tile_order() != 'ordered':
        assert torch.equal(on['k_lean'], on['k_full'])


def test_batch_of_three_equals_single_calls(S, monkeypatch, N=3000, nv=16):
    import torch
    from ssqueezepy_amd import _cwt
    monkeypatch.delenv('SSQ_DEBUG_BLOCK_PAIRED', raising=False)
    monkeypatch.delenv('SSQ_DEBUG_BLOCK_BAND', raising=False)
    xb = np.stack([two_chirps(N, seed=s) for s in (5, 6, 7)])
    wav = S.Wavelet()
    _cwt.clear_plan_cache()
    Wb, _, Db = S.cwt(xb, wav, scales='log', nv=nv, derivative=True)
    Tb, Wsb, *_ = S.ssq_cwt(xb, wav, scales='log', nv=nv)
    for b in range(len(xb)):
        _cwt.clear_plan_cache()
        W1, _, D1 = S.cwt(xb[b], wav, scales='log', nv=nv, derivative=True)
        T1, Ws1, *_ = S.ssq_cwt(xb[b], wav, scales='log', nv=nv)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.algo.startswith('blockzoom'), plan.algo
        assert torch.equal(Wb[b], W1) and torch.equal(Db[b], D1) and torch.equal(Wsb[b], Ws1), b
        assert_tx_repeat(Tb[b].cpu().numpy(), T1.cpu().numpy(), tiles=bool(plan.tile_cols), what=b)
    _cwt.clear_plan_cache()
