# -*- coding: utf-8 -*-
"""The time-reassigned synchrosqueezed CWT's three launches against the same definition composed from torch operations and
against the scatter without its LDS window -- the figures of profiles/tssq_cwt.txt and DESIGN.md section 4.5.12.

    python tools/tssq_cwt_bench.py [--repeats 5] [--dtypes float32,float64] [--signals noise,impulses,dispersive]
                                    [--small-only] [--out FILE]

Per signal and dtype, on the resident planes `W`, `Wd` of a real transform (the benchmark's workload: 'gmw', the first 300
of the 32-voice log scales, 160 000 samples; the package's own plans; `gamma`, `dmax` and the rotation tables as `tssq_cwt`
takes them), and on one launch-bound small shape:
  (a) window    `algos.time_reassign_cwt_gpu` (`ssq_time_reassign_cwt`): two clears and three launches
  (b) atomics   the same with ``window=False``: every term is two global 64-bit integer atomics
  (c) composed  the definition in torch, float64: the same two tables, the quotient, `round` (half to even), the masks,
                the complex products and `scatter_add_` on `view_as_real` of the flat plane (a float64 sum: not
                reproducible, and what (a) is compared with)
Three warm-up calls of each, then `--repeats` rounds in which the routes alternate; every call is timed on its own with
HIP events. min / median / max in ms and the ratios of the medians. The share of the terms that leave the window of
their tile, the cells on which (a) and (b) hold the same integers, and the largest ``|(a) - (c)|`` over the largest
``|(c)|`` (the project's parity norm: 1e-5 in float32, 1e-12 in float64) are printed with them, next to the bound the
fixed-point sum states for the fullest cell (its terms x ``2^-sh``).
Signals: a tone in white noise at 0 dB, an impulse train (one impulse every 997 samples: every row is impulse-like
somewhere, and the low rows' terms leave any window), and a dispersive pulse (group delay linear in frequency).
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
from ssqueezepy_amd.wavelets import Wavelet, derived_wavelets, row_frequencies, wavelet_time_std   # noqa: E402

# (N, rows)
SHAPES = [(160000, 300), (4096, 120)]
PARITY = {'float32': 1e-5, 'float64': 1e-12}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def signal(kind, N):
    t = np.arange(N)
    if kind == 'impulses':
        x = np.zeros(N)
        x[::997] = 1.
        return x
    if kind == 'dispersive':
        f = np.fft.rfftfreq(N)
        amp = np.clip((f - .04) / .04, 0., 1.) * np.clip((.46 - f) / .04, 0., 1.)
        x = np.fft.irfft(amp * np.exp(-2j * np.pi * (.3 * N * f + .4 * N * f * f)), N)
        return x / np.abs(x).max()
    return np.sqrt(2.) * np.cos(2 * np.pi * .1 * t) + np.random.default_rng(1).standard_normal(N)


def planes(kind, shape, dtype):
    """The two planes, the row vectors and the tables of `tssq_cwt` at fs = 1 on the benchmark's scales."""
    N, rows = shape
    wav = Wavelet(('gmw', {'dtype': dtype}), N=N)
    scales = np.asarray(process_scales('log', N, wav, nv=32)[:rows], dtype=dtype)
    sc_dt = _ssq_design(wav, scales, None, N, 1., None, 'peak', True)[0]
    xd = algos.to_device(signal(kind, N).astype(dtype))
    W = get_cwt_plan(wav, sc_dt, N, 'reflect', 1., True, 1).execute(xd, want_dWx=False)['Wx']
    Wd = get_cwt_plan(derived_wavelets(wav)[0], sc_dt, N, 'reflect', 1., True, 1).execute(xd)['Wx']
    sc = np.asarray(sc_dt, dtype=np.float64).reshape(-1)
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wav), 4.)
    rot = algos.cwt_rotation_tables(row_frequencies(wav, sc, 1.), N)
    return W, Wd, sc, dmax, rot


def composed(W, Wd, sc, dmax, rot, gamma, P):
    """The definition composed in torch (float64); the sum is a float64 `scatter_add_`."""
    rows, n = W.shape[-2:]
    dev = W.device
    g, t = W.to(torch.complex128), Wd.to(torch.complex128)
    gr, gi = g.real, g.imag
    e = gr * gr + gi * gi
    kept = (torch.hypot(gr, gi) >= gamma) & torch.isfinite(e)
    d = torch.round(((t.imag * gr - t.real * gi) / e) * torch.as_tensor(sc, device=dev)[:, None])
    ok = kept & (d.abs() <= torch.as_tensor(dmax, device=dev)[:, None])
    c = torch.arange(n, device=dev)
    c2 = c[None, :] + torch.where(ok, d, torch.zeros_like(d)).long()
    ok &= (c2 >= 0) & (c2 < n)
    lo, hi = rot
    z = g * (hi[:, c // P] * lo[:, c % P])
    idx = (torch.arange(rows, device=dev)[:, None] * n + c2)[ok]
    out = torch.zeros(rows * n, 2, dtype=torch.float64, device=dev)
    out.scatter_add_(0, idx[:, None].expand(-1, 2), torch.view_as_real(z[ok]))
    return torch.view_as_complex(out).view(rows, n).to(W.dtype), ok, c2, int(torch.bincount(idx, minlength=1).max())


def bench(kind, shape, dtype, repeats, emit, tile):
    W, Wd, sc, dmax, rot = planes(kind, shape, dtype)
    rows, n = W.shape
    tr, tc, hc, wc, _, P = tile
    gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)
    call = lambda **kw: algos.time_reassign_cwt_gpu(W, Wd, sc, dmax, gamma, rot=rot, return_acc=True, **kw)
    routes = {'window': lambda: call(), 'atomics': lambda: call(window=False),
              'composed': lambda: composed(W, Wd, sc, dmax, rot, gamma, P)}
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
    Tc, ok, c2, tmax = outs['composed']
    c0 = torch.arange(n, device=W.device)[None, :] // tc * tc
    away = ok & ((c2 < c0 - hc) | (c2 >= c0 - hc + wc))
    landed = int(ok.sum())
    same = float((outs['atomics'][1] == outs['window'][1]).double().mean())
    a, cc = outs['window'][0].to(torch.complex128), Tc.to(torch.complex128)
    parity = float((a - cc).abs().max() / cc.abs().max())
    emit("%s %s %d x %d, dmax %d .. %d, %d repeats" % (kind, dtype, rows, n, dmax.min(), dmax.max(), repeats))
    for name in routes:
        emit("  %-9s min %9.3f  median %9.3f  max %9.3f ms" % (name, min(ms[name]), med[name], max(ms[name])))
    emit("  composed / window = %.2f, atomics / window = %.2f (medians); terms that land %d (%.3f of the points), of them "
         "outside their tile's window %.4f; cells filled %.3f" % (med['composed'] / med['window'], med['atomics'] / med['window'],
                                                                 landed, landed / (rows * n), int(away.sum()) / max(landed, 1),
                                                                 float((cc != 0).double().mean())))
    emit("  acc equal, atomics vs window: %.6f of the cells; max |window - composed| / max |composed| = %.3e (%s %.0e)"
         % (same, parity, 'within' if parity <= PARITY[dtype] else 'BEYOND', PARITY[dtype]))
    # the fixed-point sum's own bound for the fullest cell: t 2^-sh per component, sh from the call's peak word
    ex = int(np.frexp(outs['window'][2].cpu().numpy().view(np.float64)[0])[1])
    sh = 61 - int(min(2 * int(dmax.max()) + 1, n)).bit_length() + (-ex) // 2
    emit("  the fullest cell received %d terms: its truncation bound t 2^-sh / max |composed| = %.3e (sh = %d)"
         % (tmax, tmax * 2. ** -sh / float(cc.abs().max()), sh))
    read = 2 * rows * n * (8 if dtype == 'float32' else 16)
    emit("  window: %.3f ns per point; two planes read in %.3f ms would be %.2f TB/s"
         % (med['window'] * 1e6 / (rows * n), med['window'], read / (med['window'] * 1e-3) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--small-only', action='store_true')
    ap.add_argument('--large-only', action='store_true')
    ap.add_argument('--signals', default='noise,impulses,dispersive')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tssq_cwt.txt'))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    tile = tuple(lib.ssq_time_reassign_cwt_tile(i) for i in range(6))
    emit("build %s device %s tile %d x %d halo %d window %d x %d (%d KiB) P %d"
         % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0), tile[0], tile[1], tile[2], tile[0], tile[3],
            tile[0] * tile[3] * 16 // 1024, tile[5]))
    shapes = SHAPES[-1:] if a.small_only else (SHAPES[:1] if a.large_only else SHAPES)
    for shape in shapes:
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
