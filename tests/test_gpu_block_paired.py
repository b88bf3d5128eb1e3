# -*- coding: utf-8 -*-
"""The block rows' paired LDS passes (csrc/ssq_ldsfft.h: `lds_ifft2`) on the device against one transform after the
other (`SSQ_DEBUG_BLOCK_PAIRED=0`, read when a plan is created): per plane the same butterflies on the same operands
in the same order, so `Wx`, `dWx` and every point's bin are equal bit for bit, and `Tx` as two runs on the same data
are. Shapes: the two plans of tests/test_block_paired_emulated.py -- every transform length L' = 128 .. 2048, with
workgroups that own all columns of their block, workgroups that own some, and blocks of the analytic signal -- and
the N = 6000, nv = 16 plan of tests/test_tiles_plan.py (classes P = 4096, 8192 and 16384). Each in the full build
(dWx stored) and the lean one (the benchmarked kernel), and as a plain cwt with its derivative. The runs and the
comparison are those of tests/block_builds.py; a batch against single calls is in tests/test_gpu_block_band.py."""
import pytest
from block_builds import compare_on_device

pytestmark = pytest.mark.gpu

SHAPES = ((1500, 8), (3000, 16), (6000, 16))


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


@pytest.mark.parametrize('N,nv', SHAPES)
def test_paired_passes_equal_one_transform_after_the_other(S, monkeypatch, N, nv):
    compare_on_device(S, monkeypatch, N, nv, 'SSQ_DEBUG_BLOCK_PAIRED', ('1', '0'))
