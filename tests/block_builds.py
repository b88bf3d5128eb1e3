# -*- coding: utf-8 -*-
"""Shared by the tests that compare two builds of the block rows' kernels bit for bit: the shipping build against
the one a switch of the environment selects (`SSQ_DEBUG_BLOCK_PAIRED=0`: one transform after the other;
`SSQ_DEBUG_BLOCK_BAND=0`: the band outside the transform buffer; both are read when a plan is created). `switch` is
the variable's name, a value is what it is set to, None for unset. The first part serves the device tests
(test_gpu_block_paired.py, test_gpu_block_band.py), the second the emulated ones (test_block_*_emulated.py)."""
import contextlib
import ctypes
import os
import shutil

from conftest import two_chirps, assert_tx_repeat, tile_order

SWITCHES = ('SSQ_DEBUG_BLOCK_PAIRED', 'SSQ_DEBUG_BLOCK_BAND')
LENGTHS = (128, 256, 512, 1024, 2048)


def _set(monkeypatch, switch, value):
    """Both switches unset but for `switch` = `value`."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if value is not None:
        monkeypatch.setenv(switch, value)


def _watch_plans(monkeypatch):
    """The block plans made from here on, in order (the last one: the plan of the last call)."""
    from ssqueezepy_amd import _cwt
    seen = []
    real = _cwt.plan_blocks
    monkeypatch.setattr(_cwt, 'plan_blocks', lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    return seen


# ---- on the device ---------------------------------------------------------------------------------------------
def fused(S, x, wav, nv):
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


def run_device(S, x, nv, monkeypatch, switch, value):
    """`fused` and a plain cwt with its derivative, with `switch` at `value`."""
    from ssqueezepy_amd import _cwt
    _set(monkeypatch, switch, value)
    wav = S.Wavelet()
    out = fused(S, x, wav, nv)
    Wx, sc, dWx = S.cwt(x, wav, scales='log', nv=nv, derivative=True)
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    assert plan.algo.startswith('blockzoom'), plan.algo
    out.update(Wx=Wx, dWx=dWx, algo_cwt=plan.algo)
    _cwt.clear_plan_cache()
    return out


def same(a, b, what):
    import torch
    assert a['algo'] == b['algo'] and a['algo_cwt'] == b['algo_cwt']
    for k in ('Wx', 'dWx', 'Wx_lean', 'Wx_full', 'dWx_full', 'k_lean', 'k_full'):
        assert torch.equal(a[k], b[k]), (what, k)
    for k in ('Tx_lean', 'Tx_full'):
        assert_tx_repeat(a[k], b[k], tiles=a['tiles'], what=(what, k))


def compare_on_device(S, monkeypatch, N, nv, switch, values):
    """The two settings of `switch` on two_chirps(N): equal bit for bit, and the lean and full builds agree as they
    did before. Returns the block plan of the last call."""
    import torch
    seen = _watch_plans(monkeypatch)
    x = two_chirps(N, seed=5)
    on, off = (run_device(S, x, nv, monkeypatch, switch, v) for v in values)
    same(on, off, (N, nv))
    assert torch.equal(on['Wx_lean'], on['Wx_full'])
    if on['tiles'] and tile_order() != 'ordered':
        assert torch.equal(on['k_lean'], on['k_full'])
    return seen[-1]


# ---- under the emulator ----------------------------------------------------------------------------------------
def _loaded(path):
    with open('/proc/self/maps') as fh:
        return any(line.rstrip().endswith(path) for line in fh)


@contextlib.contextmanager
def own_copy(tmp_path_factory, name, **env):
    """The package bound to a copy of the emulated library of its own, with `env` set: the emulator reads its SSQ_EMU_*
    switches once per loaded library, at its first launch, and emu_backend loads whatever SSQ_EMU_LIB names: a copy
    under another path is a library that has not launched anything yet."""
    import emu_backend
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


def emulated_module(order, tmp_path_factory, name):
    """Generator behind the emulated modules' `S` fixture. 'default-order': the emulated library as it is;
    'shuffle-reverse': a copy of its own (`name`) with the wavefronts of a workgroup in a new pseudo-random order
    after every barrier and the lanes of a wavefront in descending order."""
    import pytest
    import emu_backend
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    if order == 'default-order':
        with emu_backend.emulated() as mod:
            yield mod
    else:
        with own_copy(tmp_path_factory, name, SSQ_EMU_ORDER='shuffle', SSQ_EMU_LANES='reverse') as mod:
            yield mod


def run_emulated(S, monkeypatch, N, nv, switch, values):
    """cwt with the derivative and ssq_cwt (full and lean builds of the kernels) per value of `switch`; returns the
    outputs per value and the block plan of the last call."""
    from ssqueezepy_amd import _cwt
    seen = _watch_plans(monkeypatch)
    x = two_chirps(N, seed=5)
    wav = S.Wavelet()
    out = {}
    for value in values:
        _set(monkeypatch, switch, value)
        _cwt.clear_plan_cache()
        Wx, sc, dWx = S.cwt(x, wav, scales='log', nv=nv, derivative=True, astensor=False)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        assert plan.algo.startswith('blockzoom') and plan.block_rows > 0.5 * len(sc), plan.algo
        Tx, W2, _, _, dW2 = S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True, astensor=False)
        Tl, Wl, *_ = S.ssq_cwt(x, wav, scales='log', nv=nv, astensor=False)
        out[value] = dict(Wx=Wx, dWx=dWx, Tx=Tx, Wx_ssq=W2, dWx_ssq=dW2, Tx_lean=Tl, Wx_lean=Wl)
    _cwt.clear_plan_cache()
    return out, seen[-1]


def check_plan(name, bp):
    """The plan holds what its case is named for. whole: every workgroup owns all columns of its block, first
    column 0; mixed: blocks shared out between workgroups, rows continued past the Nyquist bin, a class over the
    analytic signal with work."""
    cls, items = bp['classes'], bp['items']
    assert sorted(items) == list(LENGTHS) and all(len(items[L]) for L in LENGTHS)   # every length, each with work
    owned = {L: (cls[items[L][:, 3], 0] // L == 4096 // L) for L in items}          # P / L' == G: the whole block
    if name == 'whole':
        assert all(o.all() for o in owned.values()) and all((items[L][:, 2] == 0).all() for L in items)
    else:
        assert sum(int((~owned[L] & (items[L][:, 2] > 0)).any()) for L in LENGTHS) >= 2
        assert bp['extended'].sum() >= 5 and cls[:, 4].sum() >= 1
        assert any(cls[items[L][:, 3], 4].any() for L in items)                      # ... and has work


def check_rows(bp):
    """rows (cls, klo, KP, L', G, pb_off) of the block plan: every length has rows; a band narrower than L' / 2 (a row's
    L' is the shortest length that holds its band, so such a row sits in the shortest transform); the two long
    transforms have zero slots, first bins that are no multiple of 256 and bands with klo mod L' + KP > L'."""
    rows = bp['rows'][bp['rows'][:, 0] >= 0]
    assert sorted(set(rows[:, 3].tolist())) == list(LENGTHS)
    assert (rows[:, 2] <= rows[:, 3]).all() and (2 * rows[:, 2] < rows[:, 3]).any()
    for L in (1024, 2048):
        big = rows[rows[:, 3] == L]
        assert (big[:, 1] % 256 != 0).any() and (big[:, 2] < L).any() and ((big[:, 1] % L) + big[:, 2] > L).any(), L
