# -*- coding: utf-8 -*-
"""The multisynchrosqueezing kernel on a table of rows against the same definition composed from torch operations,
against the plain accumulate and against the linear-table kernel -- the figures of profiles/msst_cwt.txt and DESIGN.md
section 4.5.11.

    python tools/msst_cwt_bench.py [--repeats 5] [--dtypes float32,float64] [--small-only] [--out FILE]

Per dtype and n_iter (1, 10; linear interpolation), on resident seeded planes of 300 rows x 160 000 columns over a 'log'
table (``fr[i] = 0.4 * 2^(-i / 32)``, 9.3 octaves; `Wx` standard normal; `w` the map of a chirp seen through wavelets,
``phi_j (fr_i / phi_j)^0.6`` with the ridge `phi_j` sweeping the table's range over the columns, times noise of two
rows; all finite):
  (a) kernel    `algos.multi_squeeze_cwt_gpu` (`ssq_multi_squeeze_cwt`): one kernel
  (b) composed  the definition in torch, float64: per iteration `torch.searchsorted` on the table, three `gather`s
                along the rows and a lerp on the whole plane, then `indexed_sum_onfly` on the result
  (c) plain     `indexed_sum_onfly` alone on the same planes: the accumulate kernel without `w` and the table in LDS
  (d) linear    `algos.multi_squeeze_gpu` (`ssq_multi_squeeze`) at the same shape on rows ``linspace(0, 0.5)`` with
                the like map (``phi_j + 0.6 (Sfs_i - phi_j)`` plus noise of two rows): the same kernel with the
                closed-form position in place of the search
(b) and (c) are references -- neither runs the code under test; (d) shows what the search costs. Three warm-up calls
of each, then `--repeats` rounds in which the four alternate; every call is timed on its own with HIP events. min /
median / max in ms, the ratios of the medians, each route's spread ``(max - min) / median`` -- (a) counts as faster than
(b) only if the ratio exceeds 1 + (b)'s spread, and as slower than (c) or (d) only if it is slower by more than their
spread --, and the share of cells on which (a) and (b) are equal.
Then, through `msst_cwt` itself: the share of ``|Tx|^2`` within +-1 bin of the true frequency for the three signals of
tests/msst_cwt.py at 1, 2, 5, 10 passes and at 10 passes of the nearest-row form, next to the NumPy float64
restatement's, and the reconstruction errors of `issq_cwt`.
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

SHAPE = (300, 160000)
SMALL = (65, 1024)
N_ITERS = (1, 10)
SECTION_LIMIT = 300                                             # seconds per section


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def composed(algos, Wx, w, fr, grid, n_iter):
    """The entry's definition on a descending table, whole planes at a time."""
    import torch
    rows = w.shape[-2]
    W = w.double()
    t = torch.as_tensor(fr, device=w.device)
    asc = t.flip(0).contiguous()
    lo, hi = float(fr[-1]), float(fr[0])
    have = torch.isfinite(W)
    f, moving = W.clone(), have.clone()
    for _ in range(n_iter - 1):
        inside = moving & (f >= lo) & (f <= hi)
        fi = torch.where(inside, f, torch.full_like(f, hi))
        i0 = rows - 1 - torch.searchsorted(asc, fi, right=False).clamp(1, rows - 1)
        t0 = t[i0]
        a = (fi - t0) / (t[i0 + 1] - t0)
        wa, wc = W.gather(-2, i0), W.gather(-2, i0 + 1)
        r = i0 + ((a > .5) | ((a == .5) & (i0 % 2 == 1))).long()
        g = torch.where(torch.isfinite(wa) & torch.isfinite(wc), wa + a * (wc - wa), W.gather(-2, r))
        ok = inside & torch.isfinite(g)
        moving = ok & (g != f)
        f = torch.where(ok, g, f)
    wf = torch.where(have, f, torch.full_like(f, float('inf'))).to(w.dtype)
    return algos.indexed_sum_onfly(Wx, wf, grid, 1., True)


def planes(shape, dtype):
    """``(Wx, w, fr, grid, w_lin, Sfs)``: the table's planes and, for the linear kernel, the like map on even rows."""
    import torch
    rows, n = shape
    gen = torch.Generator(device='cuda').manual_seed(1)
    rdt = getattr(torch, dtype)
    Wx = torch.view_as_complex(torch.randn((rows, n, 2), generator=gen, dtype=rdt, device='cuda'))
    fr = .4 * 2. ** (-np.arange(rows) / 32.)
    grid = fr[::-1].copy()                                       # the bins: the rows' own frequencies, ascending
    lf = torch.as_tensor(np.log2(fr), device='cuda')[:, None]
    u = torch.arange(n, device='cuda').double() / max(n - 1, 1)
    lphi = (float(np.log2(fr[-1])) + (.1 + .8 * u) * float(np.log2(fr[0] / fr[-1])))[None, :]
    noise = torch.randn((rows, n), generator=gen, dtype=torch.float64, device='cuda')
    w = torch.exp2(lphi + .6 * (lf - lphi) + (2. / 32.) * noise)
    Sfs = np.linspace(0, .5, rows).astype(dtype)
    sf = torch.as_tensor(Sfs, device='cuda').double()[:, None]
    phi = (.05 + .4 * u)[None, :]
    step = float(Sfs[1]) - float(Sfs[0])
    w_lin = (phi + .6 * (sf - phi) + 2 * step * noise).abs()
    return Wx, w.to(rdt), fr, grid, w_lin.to(rdt), Sfs


def bench(shape, dtype, repeats, emit):
    import torch
    from ssqueezepy_amd import algos
    rows, n = shape
    Wx, w, fr, grid, w_lin, Sfs = planes(shape, dtype)
    emit("%s %d x %d, %d repeats" % (dtype, rows, n, repeats))
    for n_iter in N_ITERS:
        routes = {'kernel': lambda: algos.multi_squeeze_cwt_gpu(Wx, w, fr, grid, 1., n_iter, 'linear'),
                  'composed': lambda: composed(algos, Wx, w, fr, grid, n_iter),
                  'plain': lambda: algos.indexed_sum_onfly(Wx, w, grid, 1., True),
                  'linear': lambda: algos.multi_squeeze_gpu(Wx, w_lin, Sfs, Sfs, 1., n_iter, 'linear')}
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
        moved = float((outs['kernel'] != outs['plain']).double().mean())
        emit("  n_iter %d" % n_iter)
        for name in routes:
            emit("    %-9s min %9.3f  median %9.3f  max %9.3f ms  spread %.3f"
                 % (name, min(ms[name]), med[name], max(ms[name]), spread[name]))
        emit("    composed / kernel = %.2f, kernel / plain = %.2f, kernel / linear = %.2f (medians); cells equal to the "
             "composition's: %.6f; cells that differ from one pass: %.4f"
             % (med['composed'] / med['kernel'], med['kernel'] / med['plain'], med['kernel'] / med['linear'], equal, moved))
        nbytes = rows * n * (5 if dtype == 'float32' else 10) * 4             # Wx and w read, Tx written
        emit("    kernel: %.0f MB compulsory, %.2f TB/s, %.3f ns per point"
             % (nbytes / 1e6, nbytes / (med['kernel'] * 1e-3) / 1e12, med['kernel'] * 1e6 / (rows * n)))
        del outs, routes
        torch.cuda.empty_cache()


def shares(emit):
    import ssqueezepy_amd as S
    import msst_cwt as M
    emit("msst_cwt, share of |Tx|^2 within +-1 bin of the true frequency (fs 1, 32 voices, 'log-piecewise', the interior "
         "3/4 of the columns): passes 1 | 2 | 5 | 10 | 10 nearest; then the largest |device - NumPy float64 restatement|")
    for name, (kind, n, wavelet) in M.SIGNALS.items():
        ref = M.np_shares(name)
        emit("  %-8s %-10s %s" % ('numpy64', name, ' | '.join('%.6f' % ref[k] for k in M.PASSES)))
        x, f = M.signal(kind, n)
        for dtype in ('float32', 'float64'):
            wav = M.make_wavelet(wavelet, n, dtype)
            row = []
            for n_iter, interp in M.PASSES:
                Tx, _, ssq_freqs, _ = S.msst_cwt(x, wav, n_iter=n_iter, interp=interp)
                row.append(M.share(Tx, f, ssq_freqs))
            diff = max(abs(a - ref[k]) for a, k in zip(row, M.PASSES))
            emit("  %-8s %-10s %s | %.2e" % (dtype, name, ' | '.join('%.6f' % v for v in row), diff))
    emit("issq_cwt, mean |x_rec - x| / mean |x| (linear chirp + 0.5 FM tone, N 1024, gmw): ssq_cwt | msst_cwt n_iter 10 | "
         "their ratio - 1")
    x = M.signal('chirp', 1024)[0] + .5 * M.signal('fm', 1024)[0]
    for dtype in ('float32', 'float64'):
        wav = M.make_wavelet('gmw', 1024, dtype)
        errs = []
        for Tx in (S.ssq_cwt(x, wav)[0], S.msst_cwt(x, wav, n_iter=10)[0]):
            xr = S.issq_cwt(Tx, wav).cpu().numpy().astype(np.float64)
            errs.append(float(np.abs(xr - x).mean() / np.abs(x).mean()))
        emit("  %-8s %.6e | %.6e | %.2e" % (dtype, errs[0], errs[1], errs[1] / errs[0] - 1.))


def child(section, repeats, small):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load(build_if_missing=False)

    def emit(s):
        print(s, flush=True)
    if section == 'head':
        emit("build %s device %s max_rows %d / %d, tile at %d rows: %d / %d columns"
             % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0), lib.ssq_multi_squeeze_cwt_max_rows(0),
                lib.ssq_multi_squeeze_cwt_max_rows(1), SHAPE[0], lib.ssq_multi_squeeze_cwt_tile(0, SHAPE[0]),
                lib.ssq_multi_squeeze_cwt_tile(1, SHAPE[0])))
    elif section == 'shares':
        shares(emit)
    else:
        bench(SMALL if small else SHAPE, section, repeats, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--small-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msst_cwt.txt'))
    ap.add_argument('--child')
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats, a.small_only)
    sections = ['head'] + a.dtypes.split(',') + ['shares']
    lines = []
    for section in sections:
        # a fresh process per section, under its own limit; after a failure nothing more is started
        cmd = [sys.executable, os.path.abspath(__file__), '--child', section, '--repeats', str(a.repeats)]
        try:
            r = subprocess.run(cmd + (['--small-only'] if a.small_only else []), capture_output=True, text=True,
                               timeout=SECTION_LIMIT)
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
