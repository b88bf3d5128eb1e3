# -*- coding: utf-8 -*-
"""The block rows' band staged once per workgroup in the transform buffer (csrc/ssq_cwt_blocks.hip: `BAND`; the buffer is
idle until pass 1's first store, and `lds_ifft2<L, false>` takes a barrier there) against the paired kernels with the
band outside the buffer (`SSQ_DEBUG_BLOCK_BAND=0`: three global loads per point for L' >= 1024, arrays of their own for
L' <= 512), under the CPU emulator (tests/emu/, tests/emu_backend.py). Every value is made by the same operations on the
same operands in the same order, so `Wx`, `dWx` and `Tx` -- lean and full build, and a plain cwt with its derivative --
are equal bit for bit: for every transform length L' = 128 .. 2048, for workgroups that own all columns of their block
and for those that own some, for blocks of the analytic signal, for rows whose band fills less than half of the
transform (zero slots) and rows whose first bin is no multiple of 256 (the band wraps around the transform's end).
The whole set runs twice, as tests/test_block_paired_emulated.py does: in the emulator's default order, and with the
wavefronts of a workgroup in a new pseudo-random order after every barrier and the lanes of a wavefront in descending
order -- a barrier missing between the staging and the band's reads, or between those reads and pass 1's stores, shows
there. One case runs with the emulator's LDS guard on. The library copies, the runs and the plan checks are those of
tests/block_builds.py. CPU-only."""
import numpy as np
import pytest
import emu_backend
from block_builds import check_plan, check_rows, emulated_module, own_copy, run_emulated

# (name, N, nv): the plans of tests/test_block_paired_emulated.py
#   whole: M = 4096, every row in the one class P = 4096: P / L' = G, first column 0 -- the benchmark's situation
#   mixed: M = 8192: classes P = 8192 whose blocks are shared between workgroups (c0 != 0), classes P = 4096, one of
#          them over the analytic signal
CASES = (('whole', 1500, 8), ('mixed', 3000, 16))
BAND = ('SSQ_DEBUG_BLOCK_BAND', (None, '0'))


@pytest.fixture(scope='module', params=['default-order', 'shuffle-reverse'])
def S(request, tmp_path_factory):
    yield from emulated_module(request.param, tmp_path_factory, 'libssq_hip_emu_band_perturbed.so')


@pytest.mark.parametrize('name,N,nv', CASES, ids=[c[0] for c in CASES])
def test_band_in_the_transform_buffer_equals_band_outside(S, monkeypatch, name, N, nv):
    out, bp = run_emulated(S, monkeypatch, N, nv, *BAND)
    check_plan(name, bp)
    check_rows(bp)
    for k, on in out[None].items():
        assert np.array_equal(on, out['0'][k]), (name, k)
    assert np.array_equal(out[None]['Wx_ssq'], out[None]['Wx_lean'])                # (the two builds agree, as before)


def test_staged_band_with_the_lds_guard_on(tmp_path_factory, monkeypatch):
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    name, N, nv = CASES[0]
    with own_copy(tmp_path_factory, 'libssq_hip_emu_band_guard.so', SSQ_EMU_LDSGUARD='1') as mod:
        out, bp = run_emulated(mod, monkeypatch, N, nv, *BAND)
    check_plan(name, bp)
    check_rows(bp)
    for k, on in out[None].items():
        assert np.array_equal(on, out['0'][k]), k
