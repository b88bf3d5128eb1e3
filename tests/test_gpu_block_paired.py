# -*- coding: utf-8 -*-
"""The block rows' paired LDS passes (csrc/ssq_ldsfft.h: `lds_ifft2`) on the device against one transform after the
other (`SSQ_DEBUG_BLOCK_PAIRED=0`, read when a plan is created): per plane the same butterflies on the same operands
in the same order, so `Wx`, `dWx` and every point's bin are equal bit for bit, and `Tx` as two runs on the same data
are. Shapes: the two plans of tests/test_block_paired_emulated.py -- every transform length L' = 128 .. 2048, with
workgroups that own all columns of their block, workgroups that own some, and blocks of the analytic signal -- and
the N = 6000, nv = 16 plan of tests/test_tiles_plan.py (classes P = 4096, 8192 and 16384). Each in the full build
(dWx stored) and the lean one (the benchmarked kernel), and as a plain cwt with its derivative."""
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
        done0 = plan.tiles_done() if plan.tile_cols else 0
        Tl, Wl, *_ = S.ssq_cwt(x, wav, scales='log', nv=nv)
        k_lean = kmap.clone()
        kmap.fill_(-2)
        Tf, Wf, _, _, Df = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True)
        k_full = kmap.clone()
        if plan.tile_cols:                                     # the tile kernel ran both, next to the block rows
            assert plan.tiles_done() - done0 == 2 * nsig * plan.tiles_per_signal(N)
    finally:
        if dump:
            plan.set_bin_dump(None)
    if dump:
        assert not bool((k_full[:nsig * plan.na * N] == -2).any())             # every point written
    out = dict(algo=plan.algo, Wx_lean=Wl, Wx_full=Wf, dWx_full=Df, k_lean=k_lean, k_full=k_full,
               Tx_lean=Tl.cpu().numpy(), Tx_full=Tf.cpu().numpy(), tiles=bool(plan.tile_cols))
    _cwt.clear_plan_cache()
    return out


def _run(S, x, nv, monkeypatch, paired):
    from ssqueezepy_amd import _cwt
    monkeypatch.setenv('SSQ_DEBUG_BLOCK_PAIRED', paired)
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


@pytest.mark.parametrize('N,nv', SHAPES)
def test_paired_passes_equal_one_transform_after_the_other(S, monkeypatch, N, nv):
    x = two_chirps(N, seed=5)
    on, off = (_run(S, x, nv, monkeypatch, p) for p in ('1', '0'))
    _same(on, off, (N, nv))
    import torch
    assert torch.equal(on['Wx_lean'], on['Wx_full'])           # (the two builds agree, as they did before)
    if on['tiles'] and tile_order() != 'ordered':
        assert torch.equal(on['k_lean'], on['k_full'])


def test_batch_of_three_equals_single_calls(S, monkeypatch, N=3000, nv=16):
    import torch
    from ssqueezepy_amd import _cwt
    monkeypatch.delenv('SSQ_DEBUG_BLOCK_PAIRED', raising=False)
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
