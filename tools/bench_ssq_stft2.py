# -*- coding: utf-8 -*-
"""`ssq_stft2` against `ssq_stft` of the same build, and the parts of `ssq_stft2` on their own -- the
figures of profiles/ssq_stft2.txt.

    python tools/bench_ssq_stft2.py [--shapes batch64,hop1] [--repeats 5] [--min-seconds 0.2] [--out FILE]

Per shape, in one process: a warm-up of every route, then `--repeats` rounds in which the routes
alternate; a figure is HIP events around K back-to-back calls (K chosen for >= `--min-seconds` of
work), ms per call; median and range over the rounds. The two public calls include their host side
(window cache look-up, ctypes, torch allocations); the parts are the calls `ssq_stft2` makes, on
resident data:
  stft x 3     the three plan executions (six transforms, five of them needed)
  map          `algos.phase_stft2_gpu` (`ssq_stft2_phase`): five planes read, one real plane written
  reassign     `algos.indexed_sum_onfly` (`ssq_indexed_sum`, the ordered kernel)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ssqueezepy_amd as S                                   # noqa: E402
from ssqueezepy_amd import _lib, _stft, _ssq_stft2, algos    # noqa: E402
from conftest import two_chirps                              # noqa: E402

SHAPES = {   # name: (N, n_fft, hop, B, dtype)
    'batch64': (160000, 1024, 256, 64, 'float32'),
    'hop1': (160000, 1024, 1, 1, 'float32'),
    'small': (8000, 256, 4, 2, 'float32'),                   # a quick check of the tool itself
}


def timed(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def measure(routes, repeats, min_seconds):
    """routes: {name: callable}. Returns {name: (median, lo, hi)} in ms per call."""
    ks = {}
    for name, fn in routes.items():
        fn()
        torch.cuda.synchronize()
        ks[name] = max(1, int(np.ceil(min_seconds * 1e3 / max(timed(fn, 2), 1e-3))))
    ms = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            ms[name].append(timed(fn, ks[name]))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in ms.items()}


def run_shape(name, repeats, min_seconds, emit):
    N, n_fft, hop, B, dtype = SHAPES[name]
    x = np.stack([two_chirps(N, seed=s) for s in range(B)]).astype(dtype)
    xd = torch.as_tensor(x if B > 1 else x[0], device='cuda')
    kw = dict(n_fft=n_fft, hop_len=hop, dtype=dtype)
    Tx2, Sx, ssq_freqs, Sfs, w = S.ssq_stft2(xd, get_w=True, **kw)
    rows, n = Sx.shape[-2:]
    # the parts, on the plans and arrays of that call
    g, dg, _ = _stft._window_design(None, n_fft, n_fft, hop, dtype)
    pairs = [(g, dg)] + list(_ssq_stft2._second_order_windows(g, dg, n_fft, 1.))
    plans = [_stft.get_stft_plan(N, n_fft, hop, wa, wb, 1., 'reflect', True, dtype, B) for wa, wb in pairs]
    outs = [p.execute(xd, want_dSx=True) for p in plans]
    planes = (outs[0]['Sx'], outs[0]['dSx'], outs[2]['dSx'], outs[1]['Sx'], outs[1]['dSx'])
    gamma = 10 * float(np.finfo(dtype).eps)
    const = ssq_freqs[1] - ssq_freqs[0]
    assert torch.equal(algos.phase_stft2_gpu(*planes, Sfs, gamma), w)
    del outs, Tx2
    routes = {
        'ssq_stft2': lambda: S.ssq_stft2(xd, **kw),
        'ssq_stft': lambda: S.ssq_stft(xd, **kw),
        'stft x 3': lambda: [p.execute(xd, want_dSx=True) for p in plans],
        'stft (Sx, dSx) x 1': lambda: plans[0].execute(xd, want_dSx=True),
        'map': lambda: algos.phase_stft2_gpu(*planes, Sfs, gamma),
        'reassign': lambda: algos.indexed_sum_onfly(Sx, w, ssq_freqs, const, False, False),
    }
    res = measure(routes, repeats, min_seconds)
    csize = 8 if dtype == 'float32' else 16
    points = B * rows * n
    traffic = points * (5 * csize + csize // 2)
    emit("%dx%d n_fft %d hop %d %s | Sx (%d, %d, %d), plan route %s"
         % (B, N, n_fft, hop, dtype, B, rows, n, plans[0].algo))
    for r in routes:
        emit("  %-22s median %8.3f ms  range %.3f .. %.3f" % ((r,) + res[r]))
    emit("  ssq_stft2 / ssq_stft = %.2f;  ssq_stft2 - (stft x 3 + map + reassign) = %.3f ms"
         % (res['ssq_stft2'][0] / res['ssq_stft'][0],
            res['ssq_stft2'][0] - res['stft x 3'][0] - res['map'][0] - res['reassign'][0]))
    emit("  map: %.1f MB compulsory (five planes read, w written), %.0f GB/s; %.2f ps per point"
         % (traffic / 1e6, traffic / res['map'][0] / 1e6, res['map'][0] * 1e9 / points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='batch64,hop1')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--out')
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    emit("build %s device %s" % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0)))
    for name in a.shapes.split(','):
        run_shape(name, a.repeats, a.min_seconds, emit)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
