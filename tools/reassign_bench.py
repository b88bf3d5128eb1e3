# -*- coding: utf-8 -*-
"""The reassigned spectrogram's three launches against the same definition composed from torch operations and against
the scatter without its LDS window -- the figures of profiles/reassign_stft.txt and DESIGN.md section 4.5.9.

    python tools/reassign_bench.py [--repeats 5] [--dtypes float32,float64] [--small-only] [--out FILE]

Per signal and dtype, on the resident planes `Sx`, `dSx`, `Vtg` of a real transform (Gaussian window, the package's own
plans; `gamma` as `reassign_stft` takes it):
  (a) window    `algos.reassign2d_gpu` (`ssq_reassign2d`): two clears and three launches
  (b) atomics   the same with ``window=False``: every term is a global 64-bit integer atomic
  (c) composed  the definition in torch, float64: the two quotients, `round` (half to even), the masks, `frexp` of the
                largest kept energy, `ldexp` to int64, `index_put_(accumulate=True)` on the flat int64 plane, `ldexp` back
  (d) dropped   (a) with a `gamma` above every point: the clears, the peak, the scatter's read of `Sx` and the
                conversion, no term -- what a call costs before any adding
Three warm-up calls of each, then `--repeats` rounds in which the routes alternate; every call is timed on its own with
HIP events. min / median / max in ms and the ratios of the medians. (b)'s terms are 8 bytes each: its atomic bytes per
second are quoted over the whole call and over the call less (d). The share of the terms that leave the window of
their tile, and the cells on which (a), (b) and (c) hold the same integer, are printed as a check that all computed the
same thing.
Signals: a linear chirp over 0.05 .. 0.45 cycles per sample, and white noise (the scattered worst case), 160 000
samples at hop 1 with n_fft 1024 (513 x 160 000), and a small one.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssqueezepy_amd import _lib, algos                       # noqa: E402
from ssqueezepy_amd._stft import _stft_setup                 # noqa: E402
from ssqueezepy_amd._tssq_stft import _tau_plan              # noqa: E402
from ssqueezepy_amd.configs import EPS32, EPS64              # noqa: E402

# (N, n_fft, hop)
SHAPES = [(160000, 1024, 1), (4096, 256, 1)]
TWO_PI = 6.283185307179586


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def signal(kind, N):
    t = np.arange(N)
    if kind == 'chirp':
        return np.cos(2 * np.pi * (.05 * t + .2 * t * t / N))
    return np.random.default_rng(1).standard_normal(N)


def planes(kind, shape, dtype):
    N, n_fft, hop = shape
    m = np.arange(n_fft) - n_fft // 2
    g = np.exp(-.5 * (m / (n_fft / 12.)) ** 2)
    plan, xd, fs, dtype = _stft_setup(signal(kind, N), g, n_fft, None, hop, 1., None, 'reflect', True, dtype)
    out = plan.execute(xd, want_dSx=True)
    Vtg = _tau_plan(plan, g, None, hop, fs, 'reflect', dtype, 1).execute(xd)['Sx']
    return out['Sx'], out['dSx'], Vtg


def composed(Sx, dSx, Vtg, n_fft, hop, fs, kmax, dmax, gamma):
    rows, n = Sx.shape[-2:]
    g, dg, t = Sx.to(torch.complex128), dSx.to(torch.complex128), Vtg.to(torch.complex128)
    gr, gi = g.real, g.imag
    e = gr * gr + gi * gi
    kept = (torch.hypot(gr, gi) >= gamma) & torch.isfinite(e)
    m = torch.round((-(dg.imag * gr - dg.real * gi) / e) / TWO_PI / (fs / n_fft))
    d = torch.round(((t.real * gr + t.imag * gi) / e) * (fs / hop))
    ok = kept & (m.abs() <= kmax) & (d.abs() <= dmax)
    zero = torch.zeros_like(m)
    k2 = (torch.arange(rows, device=Sx.device)[:, None] + torch.where(ok, m, zero).long()).abs()
    c2 = torch.arange(n, device=Sx.device)[None, :] + torch.where(ok, d, zero).long()
    ok &= (k2 <= rows - 1) & (c2 >= 0) & (c2 < n)
    emax = torch.where(kept, e, zero).max()
    H = (rows * min(2 * dmax + 1, n)).bit_length()
    sh = (62 - H - torch.frexp(emax)[1]).to(torch.int32)
    q = torch.ldexp(e[ok], sh).to(torch.int64)
    acc = torch.zeros(rows * n, dtype=torch.int64, device=Sx.device)
    acc.index_put_(((k2 * n + c2)[ok],), q, accumulate=True)
    Rx = torch.ldexp(acc.to(torch.float64), -sh).to(Sx.real.dtype).view(rows, n)
    return Rx, acc.view(rows, n), ok, k2, c2


def bench(kind, shape, dtype, repeats, emit, tile):
    N, n_fft, hop = shape
    Sx, dSx, Vtg = planes(kind, shape, dtype)
    rows, n = Sx.shape
    gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)
    kmax, dmax = rows - 1, algos.default_dmax(n_fft, hop)
    call = lambda **kw: algos.reassign2d_gpu(Sx, dSx, Vtg, n_fft, hop, 1., kw.pop('gamma', gamma), return_acc=True, **kw)
    routes = {'window': lambda: call(), 'atomics': lambda: call(window=False),
              'composed': lambda: composed(Sx, dSx, Vtg, n_fft, hop, 1., kmax, dmax, gamma),
              'dropped': lambda: call(gamma=1e300)}
    outs = {}
    for name, fn in routes.items():
        for _ in range(3):
            outs[name] = None
            outs[name] = fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            ms[name].append(timed(fn)[0])
    med = {name: float(np.median(ms[name])) for name in routes}
    _, acc_c, ok, k2, c2 = outs['composed']
    tr, tc, hr, hc = tile[:4]
    k, c = torch.arange(rows, device=Sx.device)[:, None], torch.arange(n, device=Sx.device)[None, :]
    r0, c0 = k // tr * tr, c // tc * tc
    away = ok & ((k2 < r0 - hr) | (k2 >= r0 + tr + hr) | (c2 < c0 - hc) | (c2 >= c0 + tc + hc))
    landed = int(ok.sum())
    same_w = float((outs['window'][1] == acc_c).double().mean())
    same_a = float((outs['atomics'][1] == outs['window'][1]).double().mean())
    emit("%s %s %d x %d, n_fft %d hop %d kmax %d dmax %d, %d repeats" % (kind, dtype, rows, n, n_fft, hop, kmax, dmax, repeats))
    for name in routes:
        emit("  %-9s min %9.3f  median %9.3f  max %9.3f ms" % (name, min(ms[name]), med[name], max(ms[name])))
    emit("  composed / window = %.2f, atomics / window = %.2f (medians); terms that land %d (%.3f of the points), of them "
         "outside their tile's window %.4f; cells filled %.3f" % (med['composed'] / med['window'], med['atomics'] / med['window'],
                                                                 landed, landed / (rows * n), int(away.sum()) / max(landed, 1),
                                                                 float((acc_c != 0).double().mean())))
    emit("  cells equal: window vs composed %.6f, atomics vs window %.6f" % (same_w, same_a))
    nbytes = 8 * landed
    excess = med['atomics'] - med['dropped']
    emit("  atomics: %.0f MB of 8-byte integer atomics, %.3f TB/s over the call, %.3f TB/s over the call less `dropped` (%.3f ms)"
         % (nbytes / 1e6, nbytes / (med['atomics'] * 1e-3) / 1e12, nbytes / (excess * 1e-3) / 1e12 if excess > 0 else float('nan'),
            excess))
    read = 3 * rows * n * (8 if dtype == 'float32' else 16)
    emit("  window: %.3f ns per point; three planes read in %.3f ms would be %.2f TB/s"
         % (med['window'] * 1e6 / (rows * n), med['window'], read / (med['window'] * 1e-3) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--small-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reassign_stft.txt'))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    tile = tuple(lib.ssq_reassign2d_tile(i) for i in range(4))
    emit("build %s device %s tile %d x %d halo %d x %d" % ((lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0)) + tile))
    for shape in (SHAPES[-1:] if a.small_only else SHAPES):
        for kind in ('chirp', 'noise'):
            for dtype in a.dtypes.split(','):
                bench(kind, shape, dtype, a.repeats, emit, tile)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
