# -*- coding: utf-8 -*-
"""The fused ConceFT entry against the same result composed from the entries that existed before it -- the figures
of profiles/conceft.txt and DESIGN.md section 4.5.5.

    python tools/conceft_bench.py [--rows 257] [--n 65536] [--tapers 3] [--proj 30] [--repeats 20] [--out FILE]

Per dtype, on resident seeded standard-normal planes, `gamma` at the median of ``|V_0|``:
  (a) fused     `algos.conceft_gpu` (`ssq_conceft`): one kernel
  (b) composed  per projection: a torch mix of the 2J planes, `algos.phase_stft_gpu`, `algos.indexed_sum_onfly`,
                `abs`, add; then the division -- nothing the parent commit lacks
Three warm-up calls of each, then `--repeats` rounds in which the two alternate; every call is timed on its own
with HIP events. min / median / max in ms and the ratio of the medians. (b) mixes in the planes' own precision, so
its float32 result is not (a)'s bit for bit; the share of cells on which the two agree to 1e-5 (float32) or 1e-12
(float64) of the largest cell is printed as a check that both computed the same thing.
Then the figures of tests/test_gpu_conceft.py::test_noisy_tone_is_no_less_concentrated_than_ssq_stft.
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


def bench(dtype, rows, n, J, Q, repeats, emit):
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
    emit("%s rows %d n %d J %d Q %d, %d repeats" % (dtype, rows, n, J, Q, repeats))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=257)
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--tapers', type=int, default=3)
    ap.add_argument('--proj', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conceft.txt'))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.load(build_if_missing=False)
    emit("build %s device %s" % (lib.ssq_build_sha().decode(), torch.cuda.get_device_name(0)))
    for dtype in ('float32', 'float64'):
        bench(dtype, a.rows, a.n, a.tapers, a.proj, a.repeats, emit)
        torch.cuda.empty_cache()
    shares(emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
