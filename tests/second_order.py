# -*- coding: utf-8 -*-
"""What the tests of the two second-order maps share (tests/test_gpu_ssq_stft2.py, tests/test_gpu_ssq_cwt2.py and
their emulated twins): the check of a map against its NumPy statement, the fixture of the parent commit's bits and
the check of the kernel's grid-stride walk. Each test module keeps its own `statement`: the definitions differ.

    python tests/second_order.py [--emulated] [--out FILE]

records tests/golden/second_order_parent.npz with the library in place (`SSQ_HIP_LIB` selects another build): run it
at the parent commit of a change to the two map kernels, commit the file, and `test_parent_bits` holds the change to it.
"""
import os
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'second_order_parent.npz')
PARENT_SHAPES = [(3, 5, 7), (2, 9, 31)]     # (B, rows, n): n odd -- a 16-byte pair straddles two rows; 105 points: a lone last one
PARENT_FS = 200.
WALK_SHAPE = (3, 33, 100003)
WALK_BLOCK = 11


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else t


def default_gamma(dtype):
    return 10 * float(np.finfo(dtype).eps)


def _above_median(v):
    """A threshold "at the median" that is no sample itself: midway between the median sample and the
    next one up (an odd count's median is a sample, and a point ON a threshold proves nothing)."""
    v = np.sort(np.asarray(v, dtype=np.float64).reshape(-1))
    k = len(v) // 2
    return .5 * (v[k] + v[k + 1])


def check_map(name, w_dev, st64, stld, gamma, chirp_tol, rdtype, w64_ref=None):
    """`w_dev` against the float64 statement within ``8 E + spacing``; returns (E, measured max). `st64`, `stld`: what
    the module's `statement` returns -- ``(w, |den| / |g|^2, |g|)`` -- evaluated in float64 and in `np.clongdouble`;
    `E`, their largest difference, is always that of the definition itself. `w64_ref`: the float64 evaluation whose
    points that fall back carry the first-order map's float32 value (`fallback32`), the reference where given."""
    from conftest import report_measured
    w64, ratio, aW = st64
    wld = stld[0]
    if w64_ref is None:
        w64_ref = w64
    fin = np.isfinite(w64) & np.isfinite(wld)
    with np.errstate(all='ignore'):
        E = float(np.abs(w64 - wld.astype(np.float64))[fin].max()) if fin.any() else 0.
        near = np.abs(aW - gamma) <= 1e-6 * gamma
        if np.isfinite(chirp_tol):
            near |= np.abs(ratio - chirp_tol) <= 1e-6 * chirp_tol
    assert near.mean() <= 1e-4, (name, float(near.mean()))
    w_ref = w64_ref.astype(rdtype)
    keep = ~near
    assert np.array_equal(np.isinf(w_dev)[keep], np.isinf(w_ref)[keep]), name
    assert not np.isnan(w_dev).any(), name
    both = keep & np.isfinite(w_ref)
    with np.errstate(all='ignore'):
        err = np.abs(w_dev.astype(np.float64) - w_ref.astype(np.float64))[both]
        bound = (8 * E + np.spacing(w_ref).astype(np.float64))[both]
    worst = float(err.max()) if err.size else 0.
    with np.errstate(all='ignore'):
        second = (np.abs(ratio) > chirp_tol) & both
    report_measured(name, E=E, max_err=worst, excluded=int(near.sum()), n_inf=int(np.isinf(w_ref).sum()),
                    n_second=int(second.sum()), n_first=int(both.sum() - second.sum()),
                    max_err_over_bound=float((err / bound).max()) if err.size else 0.)
    assert (err <= bound).all(), (name, E, worst)
    return E, worst


# ------------------------------------------------- the parent commit's bits
def _key(shape, dtype):
    return '%s_%s' % ('x'.join(map(str, shape)), dtype)


def _calls(S):
    """transform: (the entry with the row argument first, its row argument for `rows` rows in `dtype`)."""
    return {
        'stft': (lambda planes, rowarg, gamma, tol: S.phase_stft2_gpu(*planes, rowarg, gamma, tol),
                 lambda rows, dtype: np.linspace(0, .5 * PARENT_FS, rows).astype(dtype)),
        'cwt': (lambda planes, rowarg, gamma, tol: S.phase_cwt2_gpu(*planes, rowarg, PARENT_FS, gamma, tol),
                lambda rows, dtype: np.geomspace(2, 40, rows).astype(dtype)),
    }


def _statements():
    import test_gpu_ssq_stft2 as TS
    import test_gpu_ssq_cwt2 as TC
    return {'stft': lambda planes, rowarg, gamma, tol: TS.statement(*planes, rowarg, gamma, tol),
            'cwt': lambda planes, rowarg, gamma, tol: TC.statement(*planes, rowarg, PARENT_FS, gamma, tol)}


def parent_bits(S, transform, shape, dtype):
    """`w` of the entry on the fixture's inputs, and the `w` the parent commit's library gave for them."""
    with np.load(GOLDEN) as z:
        k = _key(shape, dtype)
        planes, rowarg, (gamma, tol), w_parent = z['planes_' + k], z[transform + '_rows_' + k], \
            z[transform + '_thresholds_' + k], z[transform + '_w_' + k]
    w = _np(_calls(S)[transform][0](list(planes), rowarg, float(gamma), float(tol)))
    assert w.shape == w_parent.shape and w.dtype == w_parent.dtype
    assert not np.isnan(w).any()
    return w, w_parent


def assert_parent_bits(S, transform, shape, dtype):
    w, w_parent = parent_bits(S, transform, shape, dtype)
    bits = np.uint32 if dtype == 'float32' else np.uint64
    assert np.array_equal(w.view(bits), w_parent.view(bits)), int((w.view(bits) != w_parent.view(bits)).sum())


def record_parent(S, out):
    """Seeded random planes with both thresholds at medians (`_above_median`, as
    `test_map_on_random_planes_takes_all_three_branches` chooses them), and `w` of both entries on them."""
    rng = np.random.default_rng(2025)
    calls, statements = _calls(S), _statements()
    z = {'fs': np.float64(PARENT_FS)}
    for shape in PARENT_SHAPES:
        B, rows, n = shape
        for dtype in ('float32', 'float64'):
            cdt = np.complex64 if dtype == 'float32' else np.complex128
            planes = np.stack([(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt)
                               for _ in range(5)])
            k = _key(shape, dtype)
            z['planes_' + k] = planes
            flat = [p.reshape(B * rows, n) for p in planes]
            for transform in ('stft', 'cwt'):
                rowarg = calls[transform][1](rows, dtype)
                tiled = np.tile(rowarg, B)                  # the statement's rows: (batch, rows) flattened
                _, ratio, aW = statements[transform](flat, tiled, 0., 0.)
                gamma = _above_median(aW)
                tol = _above_median(ratio[aW > gamma])
                # no point near a threshold: this library's hypot and another's cannot disagree on a branch
                assert (np.abs(aW - gamma) > 1e-6 * gamma).all() and (np.abs(ratio - tol) > 1e-6 * tol).all()
                w_ref, ratio, aW = statements[transform](flat, tiled, gamma, tol)
                n_inf, n_2 = int(np.isinf(w_ref).sum()), int(((ratio > tol) & (aW >= gamma)).sum())
                n_1 = w_ref.size - n_inf - n_2
                assert min(n_inf, n_1, n_2) >= .2 * w_ref.size, (n_inf, n_2, n_1)
                w = _np(calls[transform][0](list(planes), rowarg, gamma, tol))
                assert w.shape == shape and not np.isnan(w).any()
                assert np.array_equal(np.isinf(w).reshape(B * rows, n), np.isinf(w_ref))
                z[transform + '_rows_' + k] = rowarg
                z[transform + '_thresholds_' + k] = np.array([gamma, tol])
                z[transform + '_w_' + k] = w
    np.savez(out, **z)
    return out


# ------------------------------------------------- the walk's second trip
def walk_planes(dtype, dev, offset=0):
    """Five (B, rows, n) complex planes of `WALK_SHAPE`, standard normal, generated on the device from a seed.
    `offset=1`: views one element into their buffers, so complex64 planes start 8 bytes off a 16-byte boundary."""
    import torch
    B, rows, n = WALK_SHAPE
    gen = torch.Generator(device=dev).manual_seed(7)
    bufs = [torch.view_as_complex(torch.randn((B * rows * n + offset, 2), generator=gen, dtype=getattr(torch, dtype),
                                              device=dev)) for _ in range(5)]
    return [b[offset:].view(B, rows, n) for b in bufs]


def assert_walk(entry, planes, rowarg, den, gamma, chirp_tol):
    """`entry(planes, rowarg)` -> `w` on the whole of `WALK_SHAPE` -- more steps than a launch has threads (2^21), so
    every thread walks on by the grid's stride -- against the same entry on each block of `WALK_BLOCK` rows of one
    signal, which has fewer steps than a launch has threads. `den(planes_b, rowarg)`: the map's ``den`` for one signal,
    in torch; the three branches it and ``|g|`` select must each hold at least 10 % of a signal's points."""
    import torch
    B, rows, n = WALK_SHAPE
    assert B * rows * n > 2 * 2 * (1 << 21) and WALK_BLOCK * n < (1 << 21)
    w = entry(planes, rowarg)
    assert tuple(w.shape) == WALK_SHAPE and not bool(torch.isnan(w).any())
    for b in range(B):
        m = torch.abs(planes[0][b])
        below = m < gamma
        second = ~below & (torch.abs(den([p[b] for p in planes], rowarg)) > chirp_tol * m * m)
        shares = [float(k.sum()) / (rows * n) for k in (below, second, ~below & ~second)]
        assert min(shares) >= .1, shares
        for r0 in range(0, rows, WALK_BLOCK):
            r1 = r0 + WALK_BLOCK
            ref = entry([p[b, r0:r1] for p in planes], rowarg[r0:r1])
            assert torch.equal(w[b, r0:r1], ref.reshape(WALK_BLOCK, n)), (b, r0)


if __name__ == '__main__':
    import argparse
    import sys
    ap = argparse.ArgumentParser()
    ap.add_argument('--emulated', action='store_true', help="under the CPU emulator (tests/emu_backend.py)")
    ap.add_argument('--out', default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if a.emulated:
        import emu_backend
        with emu_backend.emulated() as mod:
            print(record_parent(mod, a.out))
    else:
        import ssqueezepy_amd
        print(record_parent(ssqueezepy_amd, a.out))
