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
there. One case runs with the emulator's LDS guard on. CPU-only."""
import contextlib
import ctypes
import os
import shutil

import numpy as np
import pytest
import emu_backend
from conftest import two_chirps

LENGTHS = (128, 256, 512, 1024, 2048)
# (name, N, nv): the plans of tests/test_block_paired_emulated.py
#   whole: M = 4096, every row in the one class P = 4096: P / L' = G, first column 0 -- the benchmark's situation
#   mixed: M = 8192: classes P = 8192 whose blocks are shared between workgroups (c0 != 0), classes P = 4096, one of
#          them over the analytic signal
CASES = (('whole', 1500, 8), ('mixed', 3000, 16))


def _loaded(path):
    with open('/proc/self/maps') as fh:
        return any(line.rstrip().endswith(path) for line in fh)


@contextlib.contextmanager
def _own_copy(tmp_path_factory, name, **env):
    """The package bound to a copy of the emulated library of its own, with `env` set: the emulator reads its SSQ_EMU_*
    switches once per loaded library, and a copy under another path is a library that has not launched anything yet."""
    names = ('SSQ_EMU_LIB',) + tuple(env)
    saved = {k: os.environ.get(k) for k in names}
    copy = str(tmp_path_factory.mktemp('emu') / name)
    shutil.copyfile(emu_backend.build(), copy)
    assert not _loaded(copy)
    os.environ.update(SSQ_EMU_LIB=copy, **env)
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


@pytest.fixture(scope='module', params=['default-order', 'shuffle-reverse'])
def S(request, tmp_path_factory):
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    if request.param == 'default-order':
        with emu_backend.emulated() as mod:
            yield mod
    else:
        with _own_copy(tmp_path_factory, 'libssq_hip_emu_band_perturbed.so', SSQ_EMU_ORDER='shuffle',
                       SSQ_EMU_LANES='reverse') as mod:
            yield mod


def _run(S, monkeypatch, N, nv):
    """cwt with the derivative and ssq_cwt (full and lean builds of the kernels), the band inside the transform buffer
    (the switch unset) and outside it; returns the outputs per setting and the block plan of the last call."""
    from ssqueezepy_amd import _cwt
    seen = []
    real = _cwt.plan_blocks
    monkeypatch.setattr(_cwt, 'plan_blocks', lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    monkeypatch.delenv('SSQ_DEBUG_BLOCK_PAIRED', raising=False)
    x = two_chirps(N, seed=5)
    wav = S.Wavelet()
    out = {}
    for band in (None, '0'):
        if band is None:
            monkeypatch.delenv('SSQ_DEBUG_BLOCK_BAND', raising=False)
        else:
            monkeypatch.setenv('SSQ_DEBUG_BLOCK_BAND', band)
        _cwt.clear_plan_cache()
        Wx, sc, dWx = S.cwt(x, wav, scales='log', nv=nv, derivative=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.algo.startswith('blockzoom') and plan.block_rows > 0.5 * len(sc), plan.algo
        Tx, W2, _, _, dW2 = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True, astensor=False)
        Tl, Wl, *_ = S.ssq_cwt(x, wav, scales='log', nv=nv, astensor=False)
        out[band] = dict(Wx=Wx, dWx=dWx, Tx=Tx, Wx_ssq=W2, dWx_ssq=dW2, Tx_lean=Tl, Wx_lean=Wl)
    _cwt.clear_plan_cache()
    return out, seen[-1]


def _check_plan(name, bp):
    cls, items, rows = bp['classes'], bp['items'], bp['rows']
    assert sorted(items) == list(LENGTHS) and all(len(items[L]) for L in LENGTHS)   # every length, each with work
    owned = {L: (cls[items[L][:, 3], 0] // L == 4096 // L) for L in items}          # P / L' == G: the whole block
    if name == 'whole':
        assert all(o.all() for o in owned.values()) and all((items[L][:, 2] == 0).all() for L in items)
    else:
        assert sum(int((~owned[L] & (items[L][:, 2] > 0)).any()) for L in LENGTHS) >= 2
        assert cls[:, 4].sum() >= 1 and any(cls[items[L][:, 3], 4].any() for L in items)
    # rows (cls, klo, KP, L', G, pb_off). A row's L' is the shortest length that holds its band, so a band narrower than
    # L' / 2 is a row of the shortest transform; the two long ones: zero slots, a first bin off the work-items' 256-element
    # stride, and a band that runs past the transform's end (klo mod L' + KP > L')
    rows = rows[rows[:, 0] >= 0]
    assert (rows[:, 2] <= rows[:, 3]).all() and (2 * rows[:, 2] < rows[:, 3]).any()
    for L in (1024, 2048):
        big = rows[rows[:, 3] == L]
        assert (big[:, 1] % 256 != 0).any() and (big[:, 2] < L).any() and ((big[:, 1] % L) + big[:, 2] > L).any(), L


@pytest.mark.parametrize('name,N,nv', CASES, ids=[c[0] for c in CASES])
def test_band_in_the_transform_buffer_equals_band_outside(S, monkeypatch, name, N, nv):
    out, bp = _run(S, monkeypatch, N, nv)
    _check_plan(name, bp)
    for k, on in out[None].items():
        assert np.array_equal(on, out['0'][k]), (name, k)
    assert np.array_equal(out[None]['Wx_ssq'], out[None]['Wx_lean'])                # (the two builds agree, as before)


def test_staged_band_with_the_lds_guard_on(tmp_path_factory, monkeypatch):
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    name, N, nv = CASES[0]
    with _own_copy(tmp_path_factory, 'libssq_hip_emu_band_guard.so', SSQ_EMU_LDSGUARD='1') as mod:
        out, bp = _run(mod, monkeypatch, N, nv)
    _check_plan(name, bp)
    for k, on in out[None].items():
        assert np.array_equal(on, out['0'][k]), k
