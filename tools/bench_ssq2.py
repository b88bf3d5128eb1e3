# -*- coding: utf-8 -*-
"""`ssq_stft2` / `ssq_cwt2` against `ssq_stft` / `ssq_cwt` of the same build, and the parts of the second-order
transform on their own -- the figures of profiles/ssq_stft2.txt and profiles/ssq_cwt2.txt.

    python tools/bench_ssq2.py --transform stft|cwt [--shapes NAME,NAME] [--repeats 5] [--min-seconds 0.2]
                               [--chirp] [--out FILE]

Per shape, in one process: a warm-up of every route, then `--repeats` rounds in which the routes
alternate; a figure is HIP events around K back-to-back calls (K chosen for >= `--min-seconds` of
work), ms per call; median and range over the rounds. The two public calls include their host side
(design, window and plan cache look-ups, ctypes, torch allocations); the parts are the calls the
second-order transform makes, on resident data:
  stft x 3 / cwt x 3   the three plan executions, each with the derivative (six planes, five of them needed)
  map                  `algos.phase_stft2_gpu` / `algos.phase_cwt2_gpu` (`ssq_stft2_phase` / `ssq_cwt2_phase`):
                       five planes read, one real plane written
  reassign             `algos.indexed_sum_onfly` (`ssq_indexed_sum`, the ordered kernel)
`--out` defaults to profiles/ssq_<transform>2.txt. `--chirp` (cwt) adds the linear-chirp figures of
tests/test_gpu_ssq_cwt2.py (the shares and the margin the test allows, from the NumPy restatement's own
float32-versus-float64 difference).
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
from ssqueezepy_amd import _lib, _cwt, _stft, _ssq_stft2, algos    # noqa: E402
from ssqueezepy_amd._ssq_cwt import _ssq_design              # noqa: E402
from ssqueezepy_amd.ssqueezing import GRID_LIN               # noqa: E402
from ssqueezepy_amd.wavelets import derived_wavelets         # noqa: E402
from conftest import two_chirps                              # noqa: E402

SHAPES = {
    'stft': {   # name: (N, n_fft, hop, B, dtype)
        'batch64': (160000, 1024, 256, 64, 'float32'),
        'hop1': (160000, 1024, 1, 1, 'float32'),
        'small': (8000, 256, 4, 2, 'float32'),               # a quick check of the tool itself
    },
    'cwt': {    # name: (N, na, B, dtype) -- the first `na` of the nv=32 log scales, as bench.py takes them
        'baseline': (160000, 300, 16, 'float32'),
        'single': (160000, 300, 1, 'float32'),
        'small': (8000, 64, 2, 'float32'),                   # a quick check of the tool itself
    },
}
DEFAULT_SHAPES = {'stft': 'batch64,hop1', 'cwt': 'baseline,single'}


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


def stft_routes(name):
    """(heading, routes, points, dtype) of an STFT shape: the parts on the plans and arrays of one `ssq_stft2` call."""
    N, n_fft, hop, B, dtype = SHAPES['stft'][name]
    x = np.stack([two_chirps(N, seed=s) for s in range(B)]).astype(dtype)
    xd = torch.as_tensor(x if B > 1 else x[0], device='cuda')
    kw = dict(n_fft=n_fft, hop_len=hop, dtype=dtype)
    Tx2, Sx, ssq_freqs, Sfs, w = S.ssq_stft2(xd, get_w=True, **kw)
    rows, n = Sx.shape[-2:]
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
    heading = ("%dx%d n_fft %d hop %d %s | Sx (%d, %d, %d), plan route %s"
               % (B, N, n_fft, hop, dtype, B, rows, n, plans[0].algo))
    return heading, routes, B * rows * n, dtype


def cwt_routes(name):
    """(heading, routes, points, dtype) of a CWT shape: the parts on the plans and arrays of one `ssq_cwt2` call."""
    N, na, B, dtype = SHAPES['cwt'][name]
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    scales = S.process_scales('log', N, wav, nv=32)[:na]
    x = np.stack([two_chirps(N, seed=s) for s in range(B)]).astype(dtype)
    xd = torch.as_tensor(x if B > 1 else x[0], device='cuda')
    kw = dict(scales=scales)
    Tx2, Wx, _, scales_out, w = S.ssq_cwt2(xd, wav, get_w=True, **kw)
    del Tx2
    scales_dt, grid_freqs, const, grid, _ = _ssq_design(wav, scales, None, N, 1., None, 'peak', True)
    plans = [_cwt.get_cwt_plan(wv, scales_dt, N, 'reflect', 1., True, B)
             for wv in (wav,) + tuple(derived_wavelets(wav))]
    outs = [p.execute(xd, want_dWx=True) for p in plans]
    planes = (outs[0]['Wx'], outs[0]['dWx'], outs[1]['Wx'], outs[1]['dWx'], outs[2]['dWx'])
    gamma = 10 * float(np.finfo(dtype).eps)
    assert torch.equal(algos.phase_cwt2_gpu(*planes, scales_dt, 1., gamma), w)
    del outs
    routes = {
        'ssq_cwt2': lambda: S.ssq_cwt2(xd, wav, **kw),
        'ssq_cwt': lambda: S.ssq_cwt(xd, wav, **kw),
        'cwt x 3': lambda: [p.execute(xd, want_dWx=True) for p in plans],
        'cwt (Wx, dWx) x 1': lambda: plans[0].execute(xd, want_dWx=True),
        'map': lambda: algos.phase_cwt2_gpu(*planes, scales_dt, 1., gamma),
        'reassign': lambda: algos.indexed_sum_onfly(Wx, w, grid_freqs, const, grid != GRID_LIN, True),
    }
    heading = "%dx%d, %d scales, %s | plan routes %s" % (B, N, len(scales_out), dtype, ', '.join(p.algo for p in plans))
    return heading, routes, B * len(scales_out) * N, dtype


def run_shape(transform, name, repeats, min_seconds, emit):
    heading, routes, points, dtype = {'stft': stft_routes, 'cwt': cwt_routes}[transform](name)
    res = measure(routes, repeats, min_seconds)
    csize = 8 if dtype == 'float32' else 16
    traffic = points * (5 * csize + csize // 2)
    second, first, plans3 = list(routes)[:3]
    emit(heading)
    for r in routes:
        emit("  %-22s median %9.3f ms  range %.3f .. %.3f" % ((r,) + res[r]))
    emit("  %s / %s = %.2f;  %s - (%s + map + reassign) = %.3f ms"
         % (second, first, res[second][0] / res[first][0], second, plans3,
            res[second][0] - res[plans3][0] - res['map'][0] - res['reassign'][0]))
    emit("  map: %.1f MB compulsory (five planes read, w written: %d bytes per point), %.0f GB/s; %.2f ps per point"
         % (traffic / 1e6, traffic // points, traffic / res['map'][0] / 1e6, res['map'][0] * 1e9 / points))


def chirp(emit):
    import test_gpu_ssq_cwt2 as T
    ref = T.chirp_reference()
    emit("linear chirp of tests/test_gpu_ssq_cwt2.py (N %(N)d, rate %(rate)g cycles/sample^2, f0 %(f0)g, nv %(nv)d): "
         "share of the interior energy in the bin of the instantaneous frequency" % T.CHIRP)
    for dtype in ('float32', 'float64'):
        wav = T.gmw(dtype)
        kw = dict(scales='log', nv=T.CHIRP['nv'], fs=1., flipud=False)
        s2 = T.ridge_share(S.ssq_cwt2(ref['x'], wav, **kw)[0].cpu().numpy(), ref['bins'], ref['cols'])
        s1 = T.ridge_share(S.ssq_cwt(ref['x'], wav, **kw)[0].cpu().numpy(), ref['bins'], ref['cols'])
        emit("  %s: ssq_cwt2 %.7f (NumPy restatement %.7f), ssq_cwt %.7f (%.7f)"
             % ((dtype, s2, ref['shares'][dtype][0], s1, ref['shares'][dtype][1])))
    emit("  margin = 4 x |restatement float32 - float64|: second order %.3g, first order %.3g"
         % (ref['margin2'], ref['margin1']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--transform', choices=('stft', 'cwt'), required=True)
    ap.add_argument('--shapes')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--chirp', action='store_true', help="cwt only")
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.chirp and a.transform != 'cwt':
        ap.error("--chirp goes with --transform cwt")
    out = a.out if a.out is not None else os.path.join(ROOT, 'profiles', 'ssq_%s2.txt' % a.transform)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    emit("build %s device %s" % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0)))
    for name in [s for s in (a.shapes or DEFAULT_SHAPES[a.transform]).split(',') if s]:
        run_shape(a.transform, name, a.repeats, a.min_seconds, emit)
        _cwt.clear_plan_cache()
        torch.cuda.empty_cache()
    if a.chirp:
        chirp(emit)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
