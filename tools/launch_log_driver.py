# -*- coding: utf-8 -*-
"""Drives the plans' host code over the emulated library (tests/emu) with the emulator's launch log on, so that two
builds of the host code can be compared by the runtime calls they make: every kernel launch (name, grid, block, dynamic
LDS bytes, stream), event record, stream wait and transform, in order.

    python tools/launch_log_driver.py LOG            # the working tree's emulated library (built if need be)
    SSQ_EMU_LIB=/other/checkout/tests/emu/_build/libssq_hip_emu.so python tools/launch_log_driver.py LOG2
    diff LOG LOG2

The other checkout needs this tree's tests/emu/hip/hip_runtime.h and tests/emu/rocfft/rocfft.h (the log lives there).
The log is appended to: one process, one file. Covers ssq_cwt on the tile path (one signal, and 17 = two launch groups,
timed and not), without the tile path, on the generic route, in float64, cwt alone and rpadded, ssq_stft / stft on the
fused, mixed-radix and rocFFT routes with the fused and the separate reassignment, and both adjoints."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main(log):
    if os.path.exists(log):
        os.remove(log)
    os.environ['SSQ_EMU_LAUNCH_LOG'] = log
    import numpy as np
    import torch
    import emu_backend
    from conftest import two_chirps

    def note(text):
        with open(log, 'a') as f:
            f.write('# %s\n' % text)

    class env:
        def __init__(self, **kw):
            self.kw = kw

        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in self.kw}
            os.environ.update(self.kw)

        def __exit__(self, *a):
            for k, v in self.old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    N, nv = 4201, 4
    x1 = two_chirps(N, seed=3).astype('float32')
    x17 = np.stack([two_chirps(N, seed=s).astype('float32') for s in range(17)])
    with emu_backend.emulated() as S:
        from ssqueezepy_amd import _cwt, _stft
        wav = S.Wavelet(('gmw', {'dtype': 'float32'}))
        wav64 = S.Wavelet(('gmw', {'dtype': 'float64'}))

        def fresh():                      # (notes which routes the plans of the last section took)
            for p in list(_cwt._PLAN_CACHE.values()):
                note('  cwt plan: %s, tile kernel %d, group %d' % (p.algo, p.tile_kernel, p.group))
            for p in list(_stft._PLAN_CACHE.values()):
                note('  stft plan: %s' % p.lib.ssq_stft_plan_algo(p._h).decode())
            _cwt.clear_plan_cache()
            _stft._PLAN_CACHE.clear()

        for name, x in (('one signal', x1), ('17 signals', x17)):
            for mode in ('f64', 'ordered'):
                fresh()
                note('ssq_cwt, tile path, %s, %s' % (name, mode))
                with env(SSQ_TILE_ORDER=mode if mode == 'ordered' else ''):
                    S.ssq_cwt(x, wav, scales='log', nv=nv)
                    S.ssq_cwt(x, wav, scales='log', nv=nv, get_dWx=True)
                    note('... two-step form (w), one signal')
                    S.ssq_cwt(x1, wav, scales='log', nv=nv, get_w=True)
        fresh()
        note('ssq_cwt, tile path, 17 signals, timed')
        S.ssq_cwt(x17, wav, scales='log', nv=nv)
        plan = next(iter(_cwt._PLAN_CACHE.values()))
        plan.timing(1)
        S.ssq_cwt(x17, wav, scales='log', nv=nv)
        plan.timing(0)
        S.ssq_cwt(x17[:3], wav, scales='log', nv=nv)
        for kw in ({'SSQ_CWT_TILES': '0'}, {'SSQ_DEBUG_CWT_ALGO': 'generic'}):
            fresh()
            note('ssq_cwt, %s' % kw)
            with env(**kw):
                S.ssq_cwt(x17, wav, scales='log', nv=nv)
                S.ssq_cwt(x1, wav, scales='log', nv=nv, get_w=True, get_dWx=True)
                plan = next(iter(_cwt._PLAN_CACHE.values()))
                plan.timing(1)
                S.ssq_cwt(x17, wav, scales='log', nv=nv)
                plan.timing(0)
        fresh()
        note('ssq_cwt, float64')
        S.ssq_cwt(x17[:3].astype('float64'), wav64, scales='log', nv=nv)
        S.ssq_cwt(x1.astype('float64'), wav64, scales='log-piecewise', nv=nv, get_w=True)
        fresh()
        note('cwt alone, with the derivative, rpadded, no padding, an odd length on the generic route')
        S.cwt(x17[:3], wav, scales='log', nv=nv)
        S.cwt(x1, wav, scales='log', nv=nv, derivative=True)
        S.cwt(x1, wav, scales='log', nv=nv, rpadded=True)
        S.cwt(x1, wav, scales='log', nv=nv, padtype=None)
        S.cwt(x1.astype('float64'), wav64, scales='log', nv=nv, derivative=True, rpadded=True)
        note('cwt adjoint')
        for dt, w in (('float32', wav), ('float64', wav64)):
            fresh()
            sc = np.asarray(S.cwt(x1.astype(dt), w, scales='log', nv=nv, astensor=False)[1])
            plan = _cwt.get_cwt_plan(w, sc, N, 'reflect', 1., True, 3)
            g = torch.ones((3, len(sc), N), dtype=torch.complex64 if dt == 'float32' else torch.complex128)
            plan.adjoint(g)
            plan.adjoint(g, g)
            plan.adjoint(None, g[0])
        xs = x17[:3, :1000]
        for route, n_fft, kw in (('fused', 256, {}), ('mixed radix', 240, {}), ('rocFFT', 256, {'SSQ_DEBUG_STFT_GENERIC': '1'})):
            with env(**kw):
                for tx in ('0', '1'):
                    fresh()
                    note('ssq_stft, %s, SSQ_DEBUG_STFT_FUSED_TX=%s' % (route, tx))
                    with env(SSQ_DEBUG_STFT_FUSED_TX=tx):
                        S.ssq_stft(xs, n_fft=n_fft, hop_len=16)
                        S.ssq_stft(xs[0], n_fft=n_fft, hop_len=16, get_w=True)
                        S.ssq_stft(xs[0], n_fft=n_fft, hop_len=16, get_dWx=True)
                        with env(SSQ_TILE_ORDER='ordered'):
                            S.ssq_stft(xs, n_fft=n_fft, hop_len=16)
                fresh()
                note('stft, %s, and its adjoint' % route)
                S.stft(xs, n_fft=n_fft, hop_len=16)
                S.stft(xs[0], n_fft=n_fft, hop_len=16, derivative=True)
                S.stft(xs[0].astype('float64'), n_fft=n_fft, hop_len=16, derivative=True)
                win = np.hanning(n_fft)
                plan = _stft.StftPlan(1000, n_fft, 16, win, np.gradient(win), max_batch=3)
                g = torch.ones((3, plan.rows, plan.n_hops), dtype=torch.complex64)
                plan.adjoint(g)
                plan.adjoint(g, g)
                plan.adjoint(None, g[0])
        fresh()
    # events by the order of their first use, not by the handle the emulator gave them: which of its timing events a plan
    # records is its own business, the order of records and waits on each stream is what two builds must share
    import re
    names = {}
    lines = [re.sub(r'event (0x[0-9a-f]+|\(nil\))', lambda m: 'event e%d' % names.setdefault(m.group(1), len(names)), ln)
             for ln in open(log)]
    open(log, 'w').writelines(lines)
    print('wrote', log)


if __name__ == '__main__':
    main(os.path.abspath(sys.argv[1]))
