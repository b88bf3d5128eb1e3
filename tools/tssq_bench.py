# -*- coding: utf-8 -*-
"""The time-reassignment kernel against the same definition composed from torch operations -- the figures of
profiles/tssq_stft.txt and DESIGN.md section 4.5.7.

    python tools/tssq_bench.py [--repeats 5] [--dtypes float32,float64] [--small-only] [--out FILE]

Per shape and dtype, on resident seeded planes (`Sx` standard normal, ``Vtg = Sx z`` with the displacement
``Re(z) cols_per_second`` spread over about +-1.5 dmax, `gamma` at the lower quartile of ``|Sx|``):
  (a) kernel    `algos.time_reassign_gpu` (`ssq_time_reassign`): one kernel
  (b) composed  the definition in torch, float64: the rotation through the same table, the division, `round` (half
                to even), the masks, `scatter_add_` along the last axis on the real and the imaginary plane, the cast
Three warm-up calls of each, then `--repeats` rounds in which the two alternate; every call is timed on its own
with HIP events. min / median / max in ms, the ratio of the medians, the composition's own spread ``(max - min) /
median`` -- the kernel counts as faster only if the ratio exceeds 1 + spread --, and the kernel's bytes per second on
its compulsory traffic: two planes read, one written. (b) adds with atomics, in no fixed order; the share of cells
on which the two agree to 1e-5 (float32) or 1e-12 (float64) of the largest cell is printed as a check that both
computed the same thing.
Shapes: 513 x 160 000 at hop 1 (one signal, n_fft 1024), 64 signals x 513 x 625 (160 000 samples at hop 256) and a
small one. On the first shape the kernel alone is also timed on its worst case: every run of 256 sources meets in
one cell, so every block of 64 takes the ordered fold.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssqueezepy_amd import _lib, algos                       # noqa: E402

GAMMA = float(np.sqrt(-2. * np.log(.75)))                    # the lower quartile of |Sx|, Sx standard normal complex
# (B, rows, n, n_fft, hop)
SHAPES = [(1, 513, 160000, 1024, 1), (64, 513, 625, 1024, 256), (1, 65, 1024, 128, 1)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def composed(Sx, Vtg, rot, n_fft, hop, cps, dmax, gamma):
    rows, n = Sx.shape[-2:]
    g, t = Sx.to(torch.complex128), Vtg.to(torch.complex128)
    gr, gi = g.real, g.imag
    s = (t.real * gr + t.imag * gi) / (gr * gr + gi * gi)
    d = torch.round(s * cps)
    c = torch.arange(n, device=Sx.device)
    ok = (torch.hypot(gr, gi) >= gamma) & (d.abs() <= dmax)
    c2 = c + torch.where(ok, d, torch.zeros_like(d)).long()
    ok &= (c2 >= 0) & (c2 < n)
    c2 = torch.where(ok, c2, c.expand_as(c2))
    p = ((torch.arange(rows, device=Sx.device) * (hop % n_fft) % n_fft)[:, None] * (c % n_fft)[None, :]) % n_fft
    v = torch.view_as_real(torch.where(ok, g * rot[p], torch.zeros_like(g)))
    out = torch.zeros_like(v)
    out[..., 0].scatter_add_(-1, c2, v[..., 0])
    out[..., 1].scatter_add_(-1, c2, v[..., 1])
    return torch.view_as_complex(out).to(Sx.dtype)


def planes(shape, dtype, pattern='noise'):
    B, rows, n, n_fft, hop = shape
    gen = torch.Generator(device='cuda').manual_seed(1)
    rdt = getattr(torch, dtype)
    dims = (rows, n) if B == 1 else (B, rows, n)
    Sx = torch.view_as_complex(torch.randn(dims + (2,), generator=gen, dtype=rdt, device='cuda'))
    dmax = algos.default_dmax(n_fft, hop)
    if pattern == 'noise':
        z = torch.view_as_complex(torch.randn(dims + (2,), generator=gen, dtype=rdt, device='cuda'))
        return Sx, Sx * z * (.75 * dmax * hop), dmax                       # fs = 1: cols_per_second = 1 / hop
    c = torch.arange(n, device='cuda')
    return Sx, Sx * ((c // 256 * 256 + 128 - c) * hop).to(rdt), dmax      # runs of 256 sources, one cell each


def bench(shape, dtype, repeats, emit):
    B, rows, n, n_fft, hop = shape
    Sx, Vtg, dmax = planes(shape, dtype)
    rot = algos.rotation_table(n_fft)
    routes = {'kernel': lambda: algos.time_reassign_gpu(Sx, Vtg, n_fft, hop, 1., GAMMA),
              'composed': lambda: composed(Sx, Vtg, rot, n_fft, hop, 1. / hop, dmax, GAMMA)}
    outs = {}
    for name, fn in routes.items():
        for _ in range(3):
            outs[name] = fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            ms[name].append(timed(fn)[0])
    top = float(outs['composed'].abs().max())
    tol = (1e-5 if dtype == 'float32' else 1e-12) * top
    agree = float(((outs['kernel'] - outs['composed']).abs() <= tol).double().mean())
    filled = float((outs['kernel'] != 0).double().mean())
    emit("%s %d x %d x %d, n_fft %d hop %d dmax %d, %d repeats" % (dtype, B, rows, n, n_fft, hop, dmax, repeats))
    for name in routes:
        emit("  %-9s min %9.3f  median %9.3f  max %9.3f ms" % (name, min(ms[name]), float(np.median(ms[name])), max(ms[name])))
    med = {name: float(np.median(ms[name])) for name in routes}
    spread = (max(ms['composed']) - min(ms['composed'])) / med['composed']
    emit("  composed / kernel = %.2f (medians); the composition's spread %.3f; cells that agree: %.6f; cells filled: %.3f"
         % (med['composed'] / med['kernel'], spread, agree, filled))
    nbytes = 3 * B * rows * n * (8 if dtype == 'float32' else 16)
    emit("  kernel: %.0f MB compulsory (two planes read, one written), %.2f TB/s, %.3f ns per point"
         % (nbytes / 1e6, nbytes / (med['kernel'] * 1e-3) / 1e12, med['kernel'] * 1e6 / (B * rows * n)))
    del outs, routes
    if shape == SHAPES[0]:
        Sx, Vtg, dmax = planes(shape, dtype, 'runs')
        fn = lambda: algos.time_reassign_gpu(Sx, Vtg, n_fft, hop, 1., 0.)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = [timed(fn)[0] for _ in range(repeats)]
        emit("  kernel, every 256 sources to one cell: min %9.3f  median %9.3f  max %9.3f ms" % (min(t), float(np.median(t)), max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--small-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tssq_stft.txt'))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    emit("build %s device %s segment %d" % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0),
                                            lib.ssq_time_reassign_segment()))
    for shape in (SHAPES[-1:] if a.small_only else SHAPES):
        for dtype in a.dtypes.split(','):
            bench(shape, dtype, a.repeats, emit)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
