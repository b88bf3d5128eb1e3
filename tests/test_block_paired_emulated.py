# -*- coding: utf-8 -*-
"""The block rows' paired LDS passes (csrc/ssq_ldsfft.h: `lds_ifft2`, Wx and dWx through each pass of the
transform as a pair) against one transform after the other (`SSQ_DEBUG_BLOCK_PAIRED=0`), under the CPU emulator
(tests/emu/, tests/emu_backend.py): per plane the same butterflies on the same operands in the same order, so
`Wx`, `dWx` and `Tx` are equal bit for bit -- for every transform length L' = 128 .. 2048, for workgroups that own
all columns of their block (P / L' = G, first column 0) and for those that own some of them (P / L' > G), and for
rows continued past the Nyquist bin (blocks of the analytic signal). The whole set runs twice: in the emulator's
default order, and with the wavefronts of a workgroup in a new pseudo-random order after every barrier and the
lanes of a wavefront in descending order (`SSQ_EMU_ORDER=shuffle`, `SSQ_EMU_LANES=reverse`) -- the two planes
share one LDS buffer inside a pass, and a barrier missing between them would show there. The library copy, the runs
and the plan checks are those of tests/block_builds.py. CPU-only."""
import numpy as np
import pytest
from block_builds import check_plan, emulated_module, run_emulated

# (name, N, nv): the inputs of test_transforms_emulated.py::test_block_classes_in_one_launch_emulated -- two_chirps,
# the default wavelet, log scales -- at the shortest lengths whose plans hold every L' and
#   whole: M = 4096, every row in the one class P = 4096: P / L' = G, one workgroup per block, first column 0
#   mixed: M = 8192: rows in a class P = 8192 (L' = 128, 256: P / L' = 2 G, a block's columns shared out between two
#          workgroups) next to classes P = 4096, one of them over the analytic signal (rows cut by the Nyquist bin,
#          continued past it)
CASES = (('whole', 1500, 8), ('mixed', 3000, 16))


@pytest.fixture(scope='module', params=['default-order', 'shuffle-reverse'])
def S(request, tmp_path_factory):
    yield from emulated_module(request.param, tmp_path_factory, 'libssq_hip_emu_perturbed.so')


@pytest.mark.parametrize('name,N,nv', CASES, ids=[c[0] for c in CASES])
def test_paired_passes_equal_one_transform_after_the_other(S, monkeypatch, name, N, nv):
    out, bp = run_emulated(S, monkeypatch, N, nv, 'SSQ_DEBUG_BLOCK_PAIRED', ('1', '0'))
    check_plan(name, bp)
    for k, on in out['1'].items():
        assert np.array_equal(on, out['0'][k]), (name, k)
    # (the two builds of the fused form agree on Wx, as they did before)
    assert np.array_equal(out['1']['Wx_ssq'], out['1']['Wx_lean'])
