# -*- coding: utf-8 -*-
"""The block rows' paired LDS passes (csrc/ssq_ldsfft.h: `lds_ifft2`, Wx and dWx through each pass of the
transform as a pair) against one transform after the other (`SSQ_DEBUG_BLOCK_PAIRED=0`), under the CPU emulator
(tests/emu/, tests/emu_backend.py): per plane the same butterflies on the same operands in the same order, so
`Wx`, `dWx` and `Tx` are equal bit for bit -- for every transform length L' = 128 .. 2048, for workgroups that own
all columns of their block (P / L' = G, first column 0) and for those that own some of them (P / L' > G), and for
rows continued past the Nyquist bin (blocks of the analytic signal). The whole set runs twice: in the emulator's
default order, and with the wavefronts of a workgroup in a new pseudo-random order after every barrier and the
lanes of a wavefront in descending order (`SSQ_EMU_ORDER=shuffle`, `SSQ_EMU_LANES=reverse`) -- the two planes
share one LDS buffer inside a pass, and a barrier missing between them would show there. CPU-only."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import emu_backend
from conftest import two_chirps

LENGTHS = (128, 256, 512, 1024, 2048)
# (name, N, nv): the inputs of test_transforms_emulated.py::test_block_classes_in_one_launch_emulated -- two_chirps,
# the default wavelet, log scales -- at the shortest lengths whose plans hold every L' and
#   whole: M = 4096, every row in the one class P = 4096: P / L' = G, one workgroup per block, first column 0
#   mixed: M = 8192: rows in a class P = 8192 (L' = 128, 256: P / L' = 2 G, a block's columns shared out between two
#          workgroups) next to classes P = 4096, one of them over the analytic signal (rows cut by the Nyquist bin,
#          continued past it)
CASES = (('whole', 1500, 8), ('mixed', 3000, 16))


def _loaded(path):
    with open('/proc/self/maps') as fh:
        return any(line.rstrip().endswith(path) for line in fh)


@pytest.fixture(scope='module', params=['default-order', 'shuffle-reverse'])
def S(request, tmp_path_factory):
    """The package bound to the emulated library; 'shuffle-reverse': to a copy of it of its own. The emulator reads
    SSQ_EMU_ORDER / SSQ_EMU_LANES once per loaded library, at its first launch, and emu_backend loads whatever
    SSQ_EMU_LIB names: a copy under another path is a library that has not launched anything yet."""
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    if request.param == 'default-order':
        with emu_backend.emulated() as mod:
            yield mod
        return
    names = ('SSQ_EMU_LIB', 'SSQ_EMU_ORDER', 'SSQ_EMU_LANES')
    saved = {k: os.environ.get(k) for k in names}
    copy = str(tmp_path_factory.mktemp('emu') / 'libssq_hip_emu_perturbed.so')
    shutil.copyfile(emu_backend.build(), copy)
    assert not _loaded(copy)
    os.environ.update(SSQ_EMU_LIB=copy, SSQ_EMU_ORDER='shuffle', SSQ_EMU_LANES='reverse')
    try:
        with emu_backend.emulated() as mod:
            assert _loaded(copy) and ctypes.CDLL(copy)._handle == mod._lib.load()._handle
            yield mod
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(S, monkeypatch, N, nv):
    """cwt with the derivative and ssq_cwt (full and lean builds of the kernels), paired passes on and off;
    returns the outputs per switch and the block plan of the last call."""
    from ssqueezepy_amd import _cwt
    seen = []
    real = _cwt.plan_blocks
    monkeypatch.setattr(_cwt, 'plan_blocks', lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    x = two_chirps(N, seed=5)
    wav = S.Wavelet()
    out = {}
    for paired in ('1', '0'):
        monkeypatch.setenv('SSQ_DEBUG_BLOCK_PAIRED', paired)
        _cwt.clear_plan_cache()
        Wx, sc, dWx = S.cwt(x, wav, scales='log', nv=nv, derivative=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.algo.startswith('blockzoom') and plan.block_rows > 0.5 * len(sc), plan.algo
        Tx, W2, _, _, dW2 = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True, astensor=False)
        Tl, Wl, *_ = S.ssq_cwt(x, wav, scales='log', nv=nv, astensor=False)
        out[paired] = dict(Wx=Wx, dWx=dWx, Tx=Tx, Wx_ssq=W2, dWx_ssq=dW2, Tx_lean=Tl, Wx_lean=Wl)
    _cwt.clear_plan_cache()
    return out, seen[-1]


@pytest.mark.parametrize('name,N,nv', CASES, ids=[c[0] for c in CASES])
def test_paired_passes_equal_one_transform_after_the_other(S, monkeypatch, name, N, nv):
    out, bp = _run(S, monkeypatch, N, nv)
    cls, items = bp['classes'], bp['items']
    assert sorted(items) == list(LENGTHS) and all(len(items[L]) for L in LENGTHS)   # every length, each with work
    owned = {L: (cls[items[L][:, 3], 0] // L == 4096 // L) for L in items}          # P / L' == G: the whole block
    if name == 'whole':
        assert all(o.all() for o in owned.values()) and all((items[L][:, 2] == 0).all() for L in items)
    else:
        assert sum(int((~owned[L] & (items[L][:, 2] > 0)).any()) for L in LENGTHS) >= 2
        assert bp['extended'].sum() >= 5 and cls[:, 4].sum() >= 1
        assert any(cls[items[L][:, 3], 4].any() for L in items)                      # ... and has work
    for k, on in out['1'].items():
        assert np.array_equal(on, out['0'][k]), (name, k)
    # (the two builds of the fused form agree on Wx, as they did before)
    assert np.array_equal(out['1']['Wx_ssq'], out['1']['Wx_lean'])
