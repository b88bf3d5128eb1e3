# -*- coding: utf-8 -*-
"""The reassigned scalogram's three launches against the same definition composed from torch operations and against
the scatter without its LDS window -- the figures of profiles/reassign_cwt.txt and DESIGN.md section 4.5.10.

    python tools/reassign_cwt_bench.py [--repeats 7] [--dtypes float32,float64] [--signals noise,chirp,impulses]
                                        [--small-only] [--out FILE]

Per signal and dtype, on the resident planes `W`, `dW`, `Wd` of a real transform (the benchmark's workload: 'gmw', the
first 300 of the 32-voice log scales, 160 000 samples; the package's own plans; `gamma`, `dmax`, the weights and the grid
as `reassign_cwt` takes them):
  (a) window    `algos.reassign_cwt_gpu` (`ssq_reassign_cwt`): two clears and three launches
  (b) atomics   the same with ``window=False``: every term is a global 64-bit integer atomic
  (c) composed  the definition in torch, float64: the two quotients, `log2` and `round` (half to even) for the bin, the
                masks, `frexp` of the largest kept term, `ldexp` to int64, `index_put_(accumulate=True)` on the flat int64
                plane, `ldexp` back
  (d) dropped   (a) with a `gamma` above every point: the clears, the peak, the scatter's read of `W` and the
                conversion, no term -- what a call costs before any adding; a route less (d) is its scatter alone
Three warm-up calls of each, then `--repeats` rounds in which the routes alternate; every call is timed on its own with
HIP events. min / median / max in ms and the ratios of the medians. The share of the terms that leave the window of
their tile, and the cells on which (a), (b) and (c) hold the same integer, are printed as a check that all computed the
same thing ((c) takes `log2` from torch: a point on a rounding boundary of the bin map may differ).
Signals: a tone in white noise at 0 dB, a linear chirp over 0.01 .. 0.4 cycles per sample, and an impulse train (one
impulse every 997 samples: every row is impulse-like somewhere, and most terms leave any window).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssqueezepy_amd import _lib, algos                       # noqa: E402
from ssqueezepy_amd._cwt import get_cwt_plan                 # noqa: E402
from ssqueezepy_amd._ssq_cwt import _ssq_design              # noqa: E402
from ssqueezepy_amd.configs import EPS32, EPS64              # noqa: E402
from ssqueezepy_amd.scales import process_scales            # noqa: E402
from ssqueezepy_amd.wavelets import Wavelet, center_frequency, derived_wavelets, wavelet_time_std   # noqa: E402

# (N, rows)
SHAPES = [(160000, 300), (4096, 120)]
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
        return np.cos(2 * np.pi * (.01 * t + .195 * t * t / N))
    if kind == 'impulses':
        x = np.zeros(N)
        x[::997] = 1.
        return x
    return np.sqrt(2.) * np.cos(2 * np.pi * .1 * t) + np.random.default_rng(1).standard_normal(N)


def planes(kind, shape, dtype):
    """The three planes and the row vectors of `reassign_cwt` at fs = 1 on the benchmark's scales."""
    N, rows = shape
    wav = Wavelet(('gmw', {'dtype': dtype}), N=N)
    scales = np.asarray(process_scales('log', N, wav, nv=32)[:rows], dtype=dtype)
    sc_dt, freqs, const, _, _ = _ssq_design(wav, scales, None, N, 1., None, 'peak', True)
    xd = algos.to_device(signal(kind, N).astype(dtype))
    out = get_cwt_plan(wav, sc_dt, N, 'reflect', 1., True, 1).execute(xd, want_dWx=True)
    Wd = get_cwt_plan(derived_wavelets(wav)[0], sc_dt, N, 'reflect', 1., True, 1).execute(xd)['Wx']
    sc = np.asarray(sc_dt, dtype=np.float64).reshape(-1)
    cst = np.broadcast_to(np.asarray(const, dtype=np.float64).reshape(-1), sc.shape).copy()
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wav), 4.)
    home = algos.reassign_cwt_home(sc, freqs, True, wc=center_frequency(wav, kind='peak-ct'))
    return out['Wx'], out['dWx'], Wd, sc, cst, dmax, np.asarray(freqs, dtype=np.float64), home


def composed(W, dW, Wd, sc, cst, dmax, freqs, gamma):
    """The definition on a log grid with `flipud`, composed in torch (float64)."""
    rows, n = W.shape[-2:]
    dev = W.device
    g, dg, t = W.to(torch.complex128), dW.to(torch.complex128), Wd.to(torch.complex128)
    gr, gi = g.real, g.imag
    e = gr * gr + gi * gi
    kept = (torch.hypot(gr, gi) >= gamma) & torch.isfinite(e)
    w = ((dg.imag * gr - dg.real * gi) / (e * TWO_PI)).abs()
    l0, dl = float(np.log2(freqs[0])), float(np.log2(freqs[1]) - np.log2(freqs[0]))
    k = rows - 1 - torch.round((torch.log2(w) - l0) / dl).nan_to_num(nan=0.).clamp(0, rows - 1).long()
    d = torch.round(((t.imag * gr - t.real * gi) / e) * torch.as_tensor(sc, device=dev)[:, None])
    ok = kept & (d.abs() <= torch.as_tensor(dmax, device=dev)[:, None])
    zero = torch.zeros_like(d)
    c2 = torch.arange(n, device=dev)[None, :] + torch.where(ok, d, zero).long()
    ok &= (c2 >= 0) & (c2 < n)
    ew = e * torch.as_tensor(cst, device=dev)[:, None]
    emax = torch.where(kept, ew, zero).max()
    H = int(np.minimum(2 * dmax.astype(np.int64) + 1, n).sum()).bit_length()
    sh = (62 - H - torch.frexp(emax)[1]).to(torch.int32)
    q = torch.ldexp(ew[ok], sh).to(torch.int64)
    acc = torch.zeros(rows * n, dtype=torch.int64, device=dev)
    acc.index_put_(((k * n + c2)[ok],), q, accumulate=True)
    Rx = torch.ldexp(acc.to(torch.float64), -sh).to(W.real.dtype).view(rows, n)
    return Rx, acc.view(rows, n), ok, k, c2


def bench(kind, shape, dtype, repeats, emit, tile):
    W, dW, Wd, sc, cst, dmax, freqs, home = planes(kind, shape, dtype)
    rows, n = W.shape
    gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)
    call = lambda **kw: algos.reassign_cwt_gpu(W, dW, Wd, sc, cst, dmax, freqs, kw.pop('gamma', gamma), flipud=True,
                                               home=home, return_acc=True, **kw)
    routes = {'window': lambda: call(), 'atomics': lambda: call(window=False),
              'composed': lambda: composed(W, dW, Wd, sc, cst, dmax, freqs, gamma),
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
    tr, tc, hr, hc, _, wr, wc = tile
    dev = W.device
    hmin = torch.as_tensor(np.array([home[i // tr * tr:i // tr * tr + tr].min() for i in range(rows)]), device=dev)[:, None]
    c0 = torch.arange(n, device=dev)[None, :] // tc * tc
    away = ok & ((k2 < hmin - hr) | (k2 >= hmin - hr + wr) | (c2 < c0 - hc) | (c2 >= c0 - hc + wc))
    landed = int(ok.sum())
    same_w = float((outs['window'][1] == acc_c).double().mean())
    same_a = float((outs['atomics'][1] == outs['window'][1]).double().mean())
    emit("%s %s %d x %d, dmax %d .. %d, %d repeats" % (kind, dtype, rows, n, dmax.min(), dmax.max(), repeats))
    for name in routes:
        emit("  %-9s min %9.3f  median %9.3f  max %9.3f ms" % (name, min(ms[name]), med[name], max(ms[name])))
    emit("  scatter alone (less `dropped`): window %.3f, atomics %.3f, composed %.3f ms"
         % tuple(med[r] - med['dropped'] for r in ('window', 'atomics', 'composed')))
    emit("  composed / window = %.2f, atomics / window = %.2f (medians); terms that land %d (%.3f of the points), of them "
         "outside their tile's window %.4f; cells filled %.3f" % (med['composed'] / med['window'], med['atomics'] / med['window'],
                                                                 landed, landed / (rows * n), int(away.sum()) / max(landed, 1),
                                                                 float((acc_c != 0).double().mean())))
    emit("  cells equal: window vs composed %.6f, atomics vs window %.6f" % (same_w, same_a))
    read = 3 * rows * n * (8 if dtype == 'float32' else 16)
    emit("  window: %.3f ns per point; three planes read in %.3f ms would be %.2f TB/s"
         % (med['window'] * 1e6 / (rows * n), med['window'], read / (med['window'] * 1e-3) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--small-only', action='store_true')
    ap.add_argument('--signals', default='noise,chirp,impulses')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reassign_cwt.txt'))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    tile = tuple(lib.ssq_reassign_cwt_tile(i) for i in range(7))
    emit("build %s device %s tile %d x %d halo %d x %d window %d x %d (%d KiB)"
         % ((lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0)) + tile[:4] + tile[5:] + (tile[5] * tile[6] * 8 // 1024,)))
    for shape in (SHAPES[-1:] if a.small_only else SHAPES):
        for kind in a.signals.split(','):
            for dtype in a.dtypes.split(','):
                bench(kind, shape, dtype, a.repeats, emit, tile)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
