# -*- coding: utf-8 -*-
"""The multisynchrosqueezing kernel against the same definition composed from torch operations and against the plain
accumulate -- the figures of profiles/msst_stft.txt and DESIGN.md section 4.5.8.

    python tools/msst_bench.py [--repeats 5] [--dtypes float32,float64] [--small-only] [--out FILE]

Per shape, dtype and n_iter (1, 4, 10; linear interpolation), on resident seeded planes (`Sx` standard normal; `w` the
map of a chirp seen through a Gaussian window, ``phi_j + 0.85 (Sfs_i - phi_j)`` with the ridge `phi_j` sweeping the
rows' range over the columns, plus noise of two rows; all finite):
  (a) kernel    `algos.multi_squeeze_gpu` (`ssq_multi_squeeze`): one kernel
  (b) composed  the definition in torch, float64: per iteration a clamp, `floor`, two `gather`s along the rows and a
                lerp on the whole plane, then `indexed_sum_onfly` on the result
  (c) plain     `indexed_sum_onfly` alone on the same planes: the accumulate kernel without the `w` slab
Three warm-up calls of each, then `--repeats` rounds in which the three alternate; every call is timed on its own with
HIP events. min / median / max in ms, the ratios of the medians, each route's spread ``(max - min) / median`` -- (a)
counts as faster than (b) only if the ratio exceeds 1 + (b)'s spread, and as slower than (c) at n_iter = 1 only if it is
slower by more than (c)'s spread --, and the share of cells on which (a) and (b) are equal.
Shapes: 513 x 160 000 (hop 1, n_fft 1024), 64 signals x 513 x 625 and 65 x 1024.
Then, through `msst_stft` itself: the share of ``|Tx|^2`` within +-1 bin of the true frequency for the linear chirp, the
quadratic chirp and the FM tone of tests/msst.py, and the reconstruction errors of `issq_stft`.
Every section runs in a process of its own under a time limit; the first one that fails ends the run.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# (B, rows, n)
SHAPES = [(1, 513, 160000), (64, 513, 625), (1, 65, 1024)]
N_ITERS = (1, 4, 10)
SECTION_LIMIT = 300                                             # seconds per section


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def composed(algos, Sx, w, Sfs, f0, df, n_iter):
    import torch
    rows = w.shape[-2]
    W = w.double()
    have = torch.isfinite(W)
    f, moving = W.clone(), have.clone()
    for _ in range(n_iter - 1):
        p = (f - f0) / df
        inside = moving & (p >= 0) & (p <= rows - 1)
        ps = p.clamp(0, rows - 1)
        i0 = ps.floor().clamp(max=rows - 2).long()
        wa, wc = W.gather(-2, i0), W.gather(-2, i0 + 1)
        g = wa + (ps - i0) * (wc - wa)
        ok = inside & torch.isfinite(g)
        moving = ok & (g != f)
        f = torch.where(ok, g, f)
    wf = torch.where(have, f, torch.full_like(f, float('inf'))).to(w.dtype)
    return algos.indexed_sum_onfly(Sx, wf, Sfs, 1.)


def planes(shape, dtype):
    import torch
    B, rows, n = shape
    gen = torch.Generator(device='cuda').manual_seed(1)
    rdt = getattr(torch, dtype)
    dims = (rows, n) if B == 1 else (B, rows, n)
    Sx = torch.view_as_complex(torch.randn(dims + (2,), generator=gen, dtype=rdt, device='cuda'))
    Sfs = np.linspace(0, .5, rows).astype(dtype)
    sf = torch.as_tensor(Sfs, device='cuda').double()[:, None]
    phi = (.1 + .3 * torch.arange(n, device='cuda').double() / max(n - 1, 1))[None, :]
    step = float(Sfs[1]) - float(Sfs[0])
    w = phi + .85 * (sf - phi) + 2 * step * torch.randn(dims, generator=gen, dtype=torch.float64, device='cuda')
    return Sx, w.abs().to(rdt), Sfs


def bench(shape, dtype, repeats, emit):
    import torch
    from ssqueezepy_amd import algos
    B, rows, n = shape
    Sx, w, Sfs = planes(shape, dtype)
    f0, df = float(np.float64(Sfs[0])), float(np.float64(Sfs[1]) - np.float64(Sfs[0]))
    emit("%s %d x %d x %d, %d repeats" % (dtype, B, rows, n, repeats))
    for n_iter in N_ITERS:
        routes = {'kernel': lambda: algos.multi_squeeze_gpu(Sx, w, Sfs, Sfs, 1., n_iter, 'linear'),
                  'composed': lambda: composed(algos, Sx, w, Sfs, f0, df, n_iter),
                  'plain': lambda: algos.indexed_sum_onfly(Sx, w, Sfs, 1.)}
        outs = {}
        for name, fn in routes.items():
            for _ in range(3):
                outs[name] = fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in routes}
        for _ in range(repeats):
            for name, fn in routes.items():
                ms[name].append(timed(fn)[0])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        equal = float((outs['kernel'] == outs['composed']).double().mean())
        emit("  n_iter %d" % n_iter)
        for name in routes:
            emit("    %-9s min %9.3f  median %9.3f  max %9.3f ms  spread %.3f"
                 % (name, min(ms[name]), med[name], max(ms[name]), spread[name]))
        emit("    composed / kernel = %.2f, kernel / plain = %.2f (medians); cells equal to the composition's: %.6f"
             % (med['composed'] / med['kernel'], med['kernel'] / med['plain'], equal))
        nbytes = B * rows * n * (5 if dtype == 'float32' else 10) * 4         # Sx and w read, Tx written
        emit("    kernel: %.0f MB compulsory, %.2f TB/s, %.3f ns per point"
             % (nbytes / 1e6, nbytes / (med['kernel'] * 1e-3) / 1e12, med['kernel'] * 1e6 / (B * rows * n)))
        del outs, routes
        torch.cuda.empty_cache()


def shares(emit):
    import ssqueezepy_amd as S
    import msst
    emit("msst_stft, share of |Tx|^2 within +-1 bin of the true frequency (N 1024, fs 1024, Gaussian window, n_fft 256, "
         "sigma 32 samples, columns [256, 768)): n_iter 1 | nearest 10 | linear 10 | linear 20")
    for dtype in ('float32', 'float64'):
        for name in ('linear', 'quadratic', 'fm'):
            x, f = msst.signal(name)
            row = []
            for n_iter, interp in ((1, 'linear'), (10, 'nearest'), (10, 'linear'), (20, 'linear')):
                Tx, _, ssq_freqs, _ = S.msst_stft(x, window=msst.gauss_window(), n_fft=msst.N_FFT, fs=msst.FS,
                                                  n_iter=n_iter, interp=interp, dtype=dtype)
                row.append(msst.share(Tx, f, ssq_freqs))
            emit("  %-8s %-9s %.3f | %.3f | %.3f | %.3f" % (dtype, name, *row))
    emit("issq_stft, mean |x_rec - x| / mean |x| (linear chirp + 0.5 FM tone, fs 1): ssq_stft | msst_stft n_iter 10")
    x = msst.signal('linear')[0] + .5 * msst.signal('fm')[0]
    for dtype in ('float32', 'float64'):
        kw = dict(window=msst.gauss_window(), n_fft=msst.N_FFT, fs=1., dtype=dtype)
        errs = []
        for Tx in (S.ssq_stft(x, **kw)[0], S.msst_stft(x, n_iter=10, **kw)[0]):
            xr = S.issq_stft(Tx, window=kw['window'], n_fft=msst.N_FFT).cpu().numpy().astype(np.float64)
            errs.append(float(np.abs(xr - x).mean() / np.abs(x).mean()))
        emit("  %-8s %.6e | %.6e" % (dtype, *errs))


def child(section, repeats):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load(build_if_missing=False)

    def emit(s):
        print(s, flush=True)
    if section == 'head':
        emit("build %s device %s max_rows %d / %d" % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0),
                                                      lib.ssq_multi_squeeze_max_rows(0), lib.ssq_multi_squeeze_max_rows(1)))
    elif section == 'shares':
        shares(emit)
    else:
        idx, dtype = section.split(':')
        bench(SHAPES[int(idx)], dtype, repeats, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--small-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msst_stft.txt'))
    ap.add_argument('--child')
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats)
    idxs = [len(SHAPES) - 1] if a.small_only else range(len(SHAPES))
    sections = ['head'] + ['%d:%s' % (i, d) for i in idxs for d in a.dtypes.split(',')] + ['shares']
    lines = []
    for section in sections:
        # a fresh process per section, under its own limit; after a failure nothing more is started
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', section, '--repeats', str(a.repeats)],
                               capture_output=True, text=True, timeout=SECTION_LIMIT)
        except subprocess.TimeoutExpired:
            print("section %s ran into its limit of %d s: stopping" % (section, SECTION_LIMIT), flush=True)
            raise SystemExit(124)
        print(r.stdout, end='', flush=True)
        if r.returncode:
            print(r.stderr[-3000:], flush=True)
            raise SystemExit("section %s failed (%d): stopping" % (section, r.returncode))
        lines += r.stdout.splitlines()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
