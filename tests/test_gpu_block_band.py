# -*- coding: utf-8 -*-
"""The block rows' band staged once per workgroup in the transform buffer (csrc/ssq_cwt_blocks.hip: `BAND`) on the device
against the paired kernels with the band outside the buffer (`SSQ_DEBUG_BLOCK_BAND=0`, read when a plan is created):
every value is made by the same operations on the same operands in the same order, so `Wx`, `dWx` and every point's bin
are equal bit for bit, and `Tx` as two runs on the same data are. Shapes: those of tests/test_gpu_block_paired.py --
every transform length L' = 128 .. 2048, workgroups that own all columns of their block and workgroups that own some,
blocks of the analytic signal, classes P = 4096, 8192 and 16384 -- each in the full build (dWx stored) and the lean one
(the benchmarked kernel), and as a plain cwt with its derivative. The plans' row tables hold what the staging has to
get right: bands narrower than half their transform (zero slots), and for L' = 1024 and 2048 first bins off the
work-items' 256-element stride and bands that run past the transform's end. The runs and the comparison are those of
tests/block_builds.py."""
import numpy as np
import pytest
from conftest import two_chirps, assert_tx_repeat
from block_builds import SWITCHES, check_rows, compare_on_device

pytestmark = pytest.mark.gpu

SHAPES = ((1500, 8), (3000, 16), (6000, 16))


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


@pytest.mark.parametrize('N,nv', SHAPES)
def test_band_in_the_transform_buffer_equals_band_outside(S, monkeypatch, N, nv):
    check_rows(compare_on_device(S, monkeypatch, N, nv, 'SSQ_DEBUG_BLOCK_BAND', (None, '0')))


def test_batch_of_three_equals_single_calls(S, monkeypatch, N=3000, nv=16):
    import torch
    from ssqueezepy_amd import _cwt
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
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
