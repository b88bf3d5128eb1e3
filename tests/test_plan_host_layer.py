# -*- coding: utf-8 -*-
"""The plans' host layer without a GPU.

1. csrc/ssq_common.h's DeviceArena and set_ssq_params in a program of their own (tests/planhost/plan_host_check.cpp),
   compiled against the emulator's headers with AddressSanitizer and UndefinedBehaviorSanitizer and run.
2. The real creates, setters and first adjoints of the emulated library with the k-th hipMalloc failing, for every k a
   successful call makes: each failing call reports an error and leaves as many live allocations as it found; an
   adjoint that failed succeeds at the next call and leaves "plan + tables" behind, no more.
CPU-only."""
import ctypes
import os
import subprocess
import numpy as np
import pytest
import emu_backend
from conftest import ROOT


def test_arena_and_set_ssq_under_sanitizers(tmp_path):
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    exe = str(tmp_path / 'plan_host_check')
    subprocess.check_call([emu_backend.CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-I', emu_backend.EMU,
                           '-I', os.path.join(ROOT, 'ssqueezepy_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'planhost', 'plan_host_check.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'PASS' in out.stdout


# ---- the emulated library's own creates, setters and first adjoints under allocation failure
class FailingAllocations:
    """The emulated library with the entries named in `sweep` called once per allocation they make: before the call
    that goes through, the k-th hipMalloc from the call's start fails, k = 1, 2, ... until none is left to fail.
    `swept[name]` is the number of failing calls made."""

    def __init__(self, lib, sweep):
        self.lib, self.sweep, self.swept = lib, set(sweep), {}
        lib.ssq_emu_live_allocations.restype = ctypes.c_long
        lib.ssq_emu_fail_malloc.restype = ctypes.c_long
        lib.ssq_emu_fail_malloc.argtypes = [ctypes.c_long]

    def live(self):
        return self.lib.ssq_emu_live_allocations()

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.sweep:
            return fn

        def call(*args):
            live0 = self.live()
            for k in range(1, 1000):
                self.lib.ssq_emu_fail_malloc(k)
                rc = fn(*args)
                left = self.lib.ssq_emu_fail_malloc(0)
                if left:                                    # the call made k - left allocations: none failed
                    assert rc == 0, self.lib.ssq_last_error()
                    self.swept[name] = self.swept.get(name, 0) + k - 1
                    return rc
                msg = self.lib.ssq_last_error()
                assert rc != 0 and msg and b'hipMalloc' in msg, "%s: allocation %d failed unnoticed (%r)" % (name, k, msg)
                assert self.live() == live0, "%s: allocation %d failed and the call left memory behind" % (name, k)
            raise AssertionError("%s never succeeded" % name)
        return call


@pytest.fixture
def failing(monkeypatch):
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as S:
        from ssqueezepy_amd import _lib, _cwt, _stft
        lib = _lib.load()

        def swept(*names):
            proxy = FailingAllocations(lib, names)
            monkeypatch.setattr(_lib, 'load', lambda *a, **k: proxy)
            return proxy
        yield S, swept
        _cwt.clear_plan_cache()
        _stft._PLAN_CACHE.clear()


@pytest.mark.parametrize('route,n_fft,env', [('fused', 256, None), ('fused-mixed-radix', 240, None),
                                             ('rocfft', 256, 'SSQ_DEBUG_STFT_GENERIC')])
def test_stft_create_and_first_adjoint_survive_every_failing_allocation(failing, monkeypatch, route, n_fft, env):
    S, swept = failing
    import torch
    from ssqueezepy_amd import _stft
    if env:
        monkeypatch.setenv(env, '1')
    win = np.hanning(n_fft)
    make = lambda: _stft.StftPlan(1000, n_fft, 16, win, np.gradient(win), max_batch=2)
    g = torch.ones((2, n_fft // 2 + 1, 1000 // 16 + 1), dtype=torch.complex64)
    # what a plan and its first adjoint leave behind when nothing fails
    proxy = swept()
    live0 = proxy.live()
    plan = make()
    assert plan.lib.ssq_stft_plan_algo(plan._h).decode() == route
    live_plan = proxy.live() - live0
    gx = plan.adjoint(g).clone()
    live_tables = proxy.live() - live0
    assert live_tables == live_plan + 2                      # (the inverse pad map: two tables)
    del plan
    assert proxy.live() == live0
    # the same with every allocation failing once
    proxy = swept('ssq_stft_plan_create', 'ssq_stft_adjoint')
    plan = make()
    assert proxy.swept['ssq_stft_plan_create'] == live_plan and proxy.live() - live0 == live_plan
    gx2 = plan.adjoint(g)
    assert proxy.swept['ssq_stft_adjoint'] >= 2 and proxy.live() - live0 == live_tables
    assert torch.equal(gx, gx2)
    del plan
    assert proxy.live() == live0


def test_cwt_create_tables_and_first_adjoint_survive_every_failing_allocation(failing, N=4201, na=64, nsig=3):
    """The plan of tests/test_gpu_tile_rows.py: block tables, exact rows and tile tables."""
    S, swept = failing
    import torch
    from ssqueezepy_amd import _cwt
    from test_gpu_tile_rows import log_scales
    wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
    scales = log_scales(N, na, wav)
    make = lambda: _cwt.CwtPlan(wav, scales, N, 'reflect', 1., True, max_batch=nsig)
    g = torch.ones((nsig, na, N), dtype=torch.complex64)
    proxy = swept()
    live0 = proxy.live()
    plan = make()
    assert plan.algo.startswith('blockzoom') and plan.algo.endswith('+tiles')
    live_plan, bytes_plan = proxy.live() - live0, plan.device_bytes
    gx = plan.adjoint(g).clone()
    live_tables = proxy.live() - live0
    assert live_tables == live_plan + 5                      # (three tables, the spectrum sums, the row workspace)
    del plan
    assert proxy.live() == live0
    proxy = swept('ssq_cwt_plan_create', 'ssq_cwt_plan_set_blocks', 'ssq_cwt_plan_set_tiles', 'ssq_cwt_adjoint')
    plan = make()
    made = sum(proxy.swept[k] for k in ('ssq_cwt_plan_create', 'ssq_cwt_plan_set_blocks', 'ssq_cwt_plan_set_tiles'))
    assert made == live_plan and proxy.live() - live0 == live_plan
    assert min(proxy.swept.values()) >= 8                    # (the create's own: bank, bands, workspaces, row lists)
    assert plan.device_bytes == bytes_plan
    gx2 = plan.adjoint(g)
    assert proxy.swept['ssq_cwt_adjoint'] == 5 and proxy.live() - live0 == live_tables
    assert torch.equal(gx, gx2)
    del plan
    assert proxy.live() == live0
