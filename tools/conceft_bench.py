# -*- coding: utf-8 -*-
"""The fused ConceFT entries against the same results composed from the entries that existed before them -- the
figures of profiles/conceft.txt and DESIGN.md section 4.5.5 and, with `--cwt`, of profiles/conceft_cwt.txt and section
4.5.6.

    python tools/conceft_bench.py [--cwt] [--rows 257] [--n 65536] [--tapers 3] [--proj 30] [--repeats 20] [--out FILE]

Per dtype, on resident seeded standard-normal planes, `gamma` at the median of ``|V_0|``:
  (a) fused     `algos.conceft_gpu` (`ssq_conceft`): one kernel
  (b) composed  per projection: a torch mix of the 2J planes, `algos.phase_stft_gpu`, `algos.indexed_sum_onfly`,
                `abs`, add; then the division -- nothing the parent commit lacks
Three warm-up calls of each, then `--repeats` rounds in which the two alternate; every call is timed on its own
with HIP events. min / median / max in ms and the ratio of the medians. (b) mixes in the planes' own precision, so
its float32 result is not (a)'s bit for bit; the share of cells on which the two agree to 1e-5 (float32) or 1e-12
(float64) of the largest cell is printed as a check that both computed the same thing.
Then the figures of tests/test_gpu_conceft.py::test_noisy_tone_is_no_less_concentrated_than_ssq_stft.

`--cwt` (300 rows unless `--rows` is given): the same protocol for the CWT form on a `log` grid of `rows` bins, 2 to
32, with the median of `w` at 8 and positive random weights:
  (a) fused     `algos.conceft_cwt_gpu` (`ssq_conceft_cwt`): one kernel
  (b) composed  per projection: a torch mix of the 2J planes, `algos.phase_cwt_gpu`, `algos.indexed_sum_onfly` with
                the weights, `abs`, add; then the division
and the figures of tests/test_gpu_conceft_cwt.py::test_noisy_tone_is_no_less_concentrated_than_ssq_cwt.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssqueezepy_amd as S                                   # noqa: E402
from ssqueezepy_amd import _lib, algos                       # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def composed(V, dV, Sfs, proj, gamma):
    acc = None
    for r in proj:
        Vq = sum(complex(r[j]) * V[j] for j in range(len(V)))
        dVq = sum(complex(r[j]) * dV[j] for j in range(len(V)))
        Tq = algos.indexed_sum_onfly(Vq, algos.phase_stft_gpu(Vq, dVq, Sfs, gamma), Sfs, 1, False, False)
        acc = torch.abs(Tq) if acc is None else acc.add_(torch.abs(Tq))
    return acc.div_(len(proj))


def composed_cwt(W, dW, cst, freqs, proj, gamma):
    acc = None
    for r in proj:
        Wq = sum(complex(r[j]) * W[j] for j in range(len(W)))
        dWq = sum(complex(r[j]) * dW[j] for j in range(len(W)))
        Tq = algos.indexed_sum_onfly(Wq, algos.phase_cwt_gpu(Wq, dWq, gamma), freqs, cst, True, False)
        acc = torch.abs(Tq) if acc is None else acc.add_(torch.abs(Tq))
    return acc.div_(len(proj))


def bench(dtype, rows, n, J, Q, repeats, emit, cwt=False):
    gen = torch.Generator(device='cuda').manual_seed(1)
    rdt = getattr(torch, dtype)
    V, dV = [[torch.view_as_complex(torch.randn((rows, n, 2), generator=gen, dtype=rdt, device='cuda'))
              for _ in range(J)] for _ in range(2)]
    dV = [p * 50. for p in dV]
    Sfs = np.linspace(0, 100., rows).astype(dtype)
    z = np.random.default_rng(0).standard_normal((Q, J, 2))
    proj = z[..., 0] + 1j * z[..., 1]
    proj /= np.sqrt((np.abs(proj) ** 2).sum(axis=1, keepdims=True))
    gamma = float(torch.abs(V[0]).median())
    routes = {'fused': lambda: algos.conceft_gpu(V, dV, Sfs, proj, Sfs, gamma),
              'composed': lambda: composed(V, dV, Sfs, proj, gamma)}
    if cwt:
        dV = [p * (8. * 2 * np.pi * np.sqrt(3.) / 50.) for p in dV]          # the median of w at 8
        freqs = 2. ** np.linspace(1., 5., rows)
        cst = np.random.default_rng(1).uniform(.5, 2., rows)
        cst_data = torch.as_tensor(cst).to(rdt)                              # (b): weights in the planes' precision
        routes = {'fused': lambda: algos.conceft_cwt_gpu(V, dV, proj, freqs, cst, gamma),
                  'composed': lambda: composed_cwt(V, dV, cst_data, freqs, proj, gamma)}
    outs = {}
    for name, fn in routes.items():
        for _ in range(3):
            outs[name] = fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            ms[name].append(timed(fn)[0])
    tol = (1e-5 if dtype == 'float32' else 1e-12) * float(outs['composed'].max())
    agree = float(((outs['fused'] - outs['composed']).abs() <= tol).double().mean())
    emit("%s%s rows %d n %d J %d Q %d, %d repeats" % ('cwt, log grid, ' if cwt else '', dtype, rows, n, J, Q, repeats))
    for name in routes:
        emit("  %-9s min %9.3f  median %9.3f  max %9.3f ms" % (name, min(ms[name]), float(np.median(ms[name])), max(ms[name])))
    emit("  composed / fused = %.2f (medians); cells that agree: %.6f"
         % (float(np.median(ms['composed'])) / float(np.median(ms['fused'])), agree))
    csize = 8 if dtype == 'float32' else 16
    emit("  fused: %.0f MB compulsory (2J planes read, Cx written), %.3f ns per point and projection"
         % (rows * n * (2 * J * csize + csize // 2) / 1e6, float(np.median(ms['fused'])) * 1e6 / (rows * n * Q)))


def shares(emit):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_conceft as T
    got = {}
    T.report_measured = lambda name, **kw: got.update(kw)
    try:
        T.test_noisy_tone_is_no_less_concentrated_than_ssq_stft(S)
    except AssertionError:
        pass
    emit("tone at row 20 in white noise at 0 dB, N 2048, n_fft 128: share of the energy within +-2 rows of the tone: "
         "conceft_stft (J 3, Q 30) %.4f, abs(ssq_stft) %.4f" % (got['conceft'], got['ssq_stft']))


def shares_cwt(emit):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_conceft_cwt as T
    got = {}
    T.report_measured = lambda name, **kw: got.update(kw)
    try:
        T.test_noisy_tone_is_no_less_concentrated_than_ssq_cwt(S)
    except AssertionError:
        pass
    emit("tone at %g cycles per sample in white noise at 0 dB, N %d, nv %d: share of |.|^2 within +-%d bins of the "
         "tone's: conceft_cwt (J 3, Q 30) %.4f, abs(ssq_cwt) %.4f"
         % (T.TONE, T.N, T.NV, T.BAND, got['conceft_cwt'], got['ssq_cwt']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cwt', action='store_true')
    ap.add_argument('--rows', type=int, default=None)
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--tapers', type=int, default=3)
    ap.add_argument('--proj', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.rows is None:
        a.rows = 300 if a.cwt else 257
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'conceft_cwt.txt' if a.cwt else 'conceft.txt')
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    emit("build %s device %s" % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0)))
    for dtype in ('float32', 'float64'):
        bench(dtype, a.rows, a.n, a.tapers, a.proj, a.repeats, emit, a.cwt)
        torch.cuda.empty_cache()
    (shares_cwt if a.cwt else shares)(emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
