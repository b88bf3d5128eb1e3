# -*- coding: utf-8 -*-
"""The host FFT layer's plan cache and scratch guard (csrc/ssq_fft.h, csrc/ssq_common.h) in a program of their own
(tests/hostfft/host_fft_check.cpp), compiled against the emulator's headers with AddressSanitizer and
UndefinedBehaviorSanitizer and run: 16 keys resident, a resident key found without `make`, the 17th key destroys
exactly 16, a failing `make` leaves no entry; every allocation of the guard freed at an early return. CPU-only."""
import os
import subprocess
import pytest
import emu_backend
from conftest import ROOT


def test_plan_cache_and_scratch_guard_under_sanitizers(tmp_path):
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    exe = str(tmp_path / 'host_fft_check')
    subprocess.check_call([emu_backend.CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-I', emu_backend.EMU,
                           '-I', os.path.join(ROOT, 'ssqueezepy_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'hostfft', 'host_fft_check.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'PASS' in out.stdout
