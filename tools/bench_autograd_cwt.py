# -*- coding: utf-8 -*-
"""`cwt` / `ssq_cwt` forward + backward on the device: the plan-level adjoint (`ssq_cwt_adjoint`)
against the route it replaced and against a plain torch.fft statement -- the figures of
profiles/autograd_cwt.txt.

    python tools/bench_autograd_cwt.py [--shapes bench16,bench1,f64] [--repeats 5] [--min-seconds 0.3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_autograd_cwt.py --trace

Routes, alternating inside every repeat, same process:
  (a) ours    `S.cwt` / `S.ssq_cwt` of a tensor that requires grad, then `.backward(G)` with resident G
  (b) parent  the same calls with `CwtPlan.adjoint` replaced by the route of the commit before the
              plan-level adjoint, restated here: per signal a zero-extended (na, M) copy, `ssq_icwt2`
              with `plan.dense_bank`, `torch.segment_reduce` over `plan.pad_segments` (it has no gradient
              for `dWx`)
  (c) torch   pad gather, torch.fft.fft, dense bank, (1j m_k), torch.fft.ifft, slice; `.backward(G)`
HIP events around K calls (K chosen for >= `--min-seconds` of work per figure), three warm-up calls per
shape and route; ms per call: median (min - max) of the repeats. One JSON line per shape at the end.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ssqueezepy_amd as S                       # noqa: E402
from ssqueezepy_amd import _cwt, _lib, algos     # noqa: E402
from ssqueezepy_amd._lib import check, F32, F64  # noqa: E402
from conftest import two_chirps                  # noqa: E402

DEV = torch.device('cuda')
SHAPES = {   # name: (N, na, dtype, B)
    'bench16': (160000, 300, 'float32', 16),
    'bench1': (160000, 300, 'float32', 1),
    'f64': (1048576, 512, 'float64', 1),
    'small': (4000, 60, 'float32', 4),            # a quick check of the tool itself
}


def parent_adjoint(plan, gW, gdW=None, rpadded=False):
    """`CwtPlan.adjoint` as it was before `ssq_cwt_adjoint` (gW only)."""
    cdt = torch.complex64 if plan.dtype == 'float32' else torch.complex128
    rdt = torch.float32 if plan.dtype == 'float32' else torch.float64
    assert gdW is None, "the parent's route has no gradient for dWx"
    batched = gW.ndim == 3
    g3 = gW if batched else gW[None]
    dev = g3.device
    psih = plan.dense_bank(dev)
    order, counts = plan.pad_segments(dev)
    code = F32 if plan.dtype == 'float32' else F64
    out = torch.zeros((g3.shape[0], plan.N), dtype=rdt, device=dev)
    v = torch.empty(plan.M, dtype=rdt, device=dev)
    for b in range(g3.shape[0]):
        if rpadded:
            Gp = g3[b].to(cdt).contiguous().clone()
        else:
            Gp = torch.zeros((plan.na, plan.M), dtype=cdt, device=dev)
            Gp[:, plan.n1:plan.n1 + plan.N] = g3[b]
        check(plan.lib.ssq_icwt2(code, Gp.data_ptr(), psih.data_ptr(), v.data_ptr(),
                                 plan.na, plan.M, algos.stream()))
        out[b] = torch.segment_reduce(v[order], 'sum', lengths=counts)
    return out if batched else out[0]


class parent_route():
    """Within the block the plan's backward takes the parent's route."""

    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        p = self.plan
        p.adjoint = lambda gW=None, gdW=None, rpadded=False: parent_adjoint(p, gW, gdW, rpadded)

    def __exit__(self, *a):
        del self.plan.adjoint


def multiplier(plan):
    rdt = np.dtype(plan.dtype).type
    k = np.arange(plan.M)
    ks = np.where(k <= plan.M // 2, k, k - plan.M).astype(np.float64)
    return (ks * (2.0 * 3.141592653589793 / plan.M)).astype(rdt) * (rdt(1) / rdt(plan.dt))


def torch_cwt(plan, x, derivative):
    psih, src = plan.dense_bank(x.device), plan.pad_sources(x.device)
    xp = torch.where(src >= 0, x[..., src.clamp(min=0)], torch.zeros((), dtype=x.dtype, device=x.device))
    xh = torch.fft.fft(xp, dim=-1)[..., None, :]
    sl = slice(plan.n1, plan.n1 + plan.N)
    W = torch.fft.ifft(psih * xh, dim=-1)[..., sl]
    if not derivative:
        return W, None
    m = torch.as_tensor(multiplier(plan), device=x.device)
    return W, torch.fft.ifft(psih * (1j * m) * xh, dim=-1)[..., sl]


def timed(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def measure(routes, repeats, min_seconds):
    """routes: {name: fn}. Returns {name: (median, min, max)} in ms per call."""
    ks = {}
    for name, fn in routes.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ks[name] = max(1, int(math.ceil(min_seconds * 1e3 / max(timed(fn, 1), 1e-3))))
    ms = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            ms[name].append(timed(fn, ks[name]))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}


def peak_bytes(plan, fn):
    """Peak device memory while `fn` runs: the plan's own (outside torch's allocator) + torch's peak."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return plan.device_bytes + torch.cuda.max_memory_allocated(), plan.device_bytes, base


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def fmt(t):
    return "%.3f (%.3f - %.3f)" % t


def run_shape(name, repeats, min_seconds):
    N, na, dtype, B = SHAPES[name]
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    cdt = torch.complex64 if dtype == 'float32' else torch.complex128
    wav = S.Wavelet(('gmw', {'dtype': dtype}))
    scales = S.process_scales('log', N, wav, nv=32)[:na]
    xb = np.stack([two_chirps(N, s) for s in range(B)])
    x0 = torch.as_tensor(xb if B > 1 else xb[0], dtype=rdt, device=DEV)
    shape = ((B,) if B > 1 else ()) + (na, N)
    gen = torch.Generator(device=DEV).manual_seed(1)
    G = torch.randn(shape, dtype=cdt, device=DEV, generator=gen)
    G2 = torch.randn(shape, dtype=cdt, device=DEV, generator=gen)
    _cwt.clear_plan_cache()
    S.cwt(x0, wav, scales=scales)
    plan = next(iter(_cwt._PLAN_CACHE.values()))
    rec = {"shape": name, "N": N, "na": na, "dtype": dtype, "B": B, "M": plan.M, "algo": plan.algo,
           "bank_nnz": plan.bank_nnz, "build_sha": _lib.load(build_if_missing=False).ssq_build_sha().decode()}

    def cwt_ours(derivative=False):
        x = x0.clone().requires_grad_(True)
        out = S.cwt(x, wav, scales=scales, derivative=derivative)
        if derivative:
            torch.autograd.backward([out[0], out[2]], [G, G2])
        else:
            out[0].backward(G)
        return x.grad

    def cwt_parent():
        with parent_route(plan):
            return cwt_ours()

    def cwt_torch(derivative=False):
        x = x0.clone().requires_grad_(True)
        W, dW = torch_cwt(plan, x, derivative)
        if derivative:
            torch.autograd.backward([W, dW], [G, G2])
        else:
            W.backward(G)
        return x.grad

    def ssq_ours():
        x = x0.clone().requires_grad_(True)
        Tx = S.ssq_cwt(x, wav, scales=scales)[0]
        Tx.backward(G)
        return x.grad

    # gradients first (and the dense bank of routes b, c exists before anything is timed)
    ga, gb, gc = cwt_ours(), cwt_parent(), cwt_torch()
    rec["grad_a_vs_b"], rec["grad_a_vs_c"], rec["grad_b_vs_c"] = relmax(ga, gb), relmax(ga, gc), relmax(gb, gc)
    rec["grad_dWx_a_vs_c"] = relmax(cwt_ours(True), cwt_torch(True))
    sa = ssq_ours()
    plan2 = list(_cwt._PLAN_CACHE.values())[-1]        # the plan `ssq_cwt` used (the same one for the same scales)

    def ssq_parent2():
        with parent_route(plan2):
            return ssq_ours()
    rec["grad_ssq_a_vs_b"] = relmax(sa, ssq_parent2())
    del ga, gb, gc, sa

    res = measure({
        "cwt a": cwt_ours, "cwt b": cwt_parent, "cwt c": cwt_torch,
        "cwt+dWx a": lambda: cwt_ours(True), "cwt+dWx c": lambda: cwt_torch(True),
        "ssq_cwt a": ssq_ours, "ssq_cwt b": ssq_parent2,
        "adjoint a": lambda: plan.adjoint(G), "adjoint b": lambda: parent_adjoint(plan, G),
        "adjoint+dWx a": lambda: plan.adjoint(G, G2),
        "forward": lambda: plan.execute(x0),
    }, repeats, min_seconds)
    rec["ms"] = {k: list(v) for k, v in res.items()}
    pa = peak_bytes(plan, lambda: plan.adjoint(G))
    pa2 = peak_bytes(plan, lambda: plan.adjoint(G, G2))
    pb = peak_bytes(plan, lambda: parent_adjoint(plan, G))
    rec["peak_bytes"] = {"adjoint a": pa[0], "adjoint+dWx a": pa2[0], "adjoint b": pb[0],
                         "plan": pa[1], "resident before the call (x, G, G2, dense bank of b / c)": pa[2]}
    # the multiply-accumulate's compulsory bytes per signal: F (and G) inside the bands, the bank, the bins' sums
    cs = 8 if dtype == 'float32' else 16
    cover = np.zeros(plan.M + 1, dtype=np.int64)
    lens = np.diff(plan._bank[1])
    np.add.at(cover, plan._bank[2][lens > 0], 1)
    np.add.at(cover, (plan._bank[2] + lens)[lens > 0], -1)
    touched = int(np.count_nonzero(np.cumsum(cover)[:-1]))
    rec["mac_bytes_per_signal"] = {"gW": plan.bank_nnz * (cs + cs // 2) + 2 * touched * cs,
                                   "gW+gdW": plan.bank_nnz * (2 * cs + cs // 2) + 2 * touched * cs,
                                   "bins touched": touched}
    print("\n%s: N = %d, %d scales, %s, B = %d (M = %d, forward: %s)" % (name, N, na, dtype, B, plan.M, plan.algo))
    for k, v in res.items():
        print("  %-16s %s ms" % (k, fmt(v)))
    print("  peak bytes: adjoint a %.3f GB, with dWx %.3f GB, adjoint b %.3f GB (plan %.3f GB)"
          % (pa[0] / 1e9, pa2[0] / 1e9, pb[0] / 1e9, pa[1] / 1e9))
    print("  gradients: a vs b %.2e, a vs c %.2e, b vs c %.2e, with dWx a vs c %.2e, ssq_cwt a vs b %.2e"
          % (rec["grad_a_vs_b"], rec["grad_a_vs_c"], rec["grad_b_vs_c"], rec["grad_dWx_a_vs_c"], rec["grad_ssq_a_vs_b"]))
    print(json.dumps(rec), flush=True)
    _cwt.clear_plan_cache()
    del G, G2
    torch.cuda.empty_cache()


def run_trace():
    """Six adjoint calls per route at the benchmark shape, one signal and sixteen: for a kernel trace."""
    N, na = 160000, 300
    wav = S.Wavelet()
    scales = np.asarray(S.process_scales('log', N, wav, nv=32)[:na], dtype='float32')
    plan = _cwt.get_cwt_plan(wav, scales, N, 'reflect', 1., True, 16, cache=False)
    for B in (1, 16):
        G = torch.randn((B, na, N), dtype=torch.complex64, device=DEV)
        G2 = torch.randn((B, na, N), dtype=torch.complex64, device=DEV)
        for _ in range(6):
            plan.adjoint(G)
        for _ in range(6):
            plan.adjoint(G, G2)
        torch.cuda.synchronize()
    print("trace run done")


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='bench16,bench1,f64')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if args.trace:
        run_trace()
    else:
        for nm in args.shapes.split(','):
            run_shape(nm, args.repeats, args.min_seconds)
