# -*- coding: utf-8 -*-
"""What the tests of the ridge-tracking kernels share (tests/test_gpu_ridge_shapes.py, its emulated twins in
tests/test_ridge_kernels_emulated.py and tests/test_ridge_cases_design.py): seeded `(E, sc, penalty)` inputs of four
kinds, the shapes by type combination, the row limits of `ssq_ridge_track`, a count of the backward pass's matching
rows, a plain NumPy statement of `extract_ridges`, and the comparisons themselves, written over a small driver so
that the GPU module and the emulated twins assert the same things.

The tracking is index work on rounded sums: everything here is compared bit for bit (`array_equal`).
"""
import numpy as np

# ---- row limits --------------------------------------------------------------------------------
# include/ssq_hip.h, beside ssq_ridge_track: "at most 4549 rows of float32 data, 2408 rows of float64 data with
# float32 penalties, 2274 rows of float64 data with float64 penalties" (tests/test_ridge_cases_design.py reads the
# header and the README for these figures)
MAX_ROWS = {('float32', 'float32'): 4549, ('float64', 'float32'): 2408, ('float64', 'float64'): 2274}
COMBOS = tuple(MAX_ROWS)
KINDS = ('ties', 'flat', 'rounded', 'random')
SEED = 3

# (rows, n) by (data type, penalty type): the forward variants of ridge_geometry on both sides of their boundaries,
# the LDS tiles as they shrink, S == 1 (from 2049 rows), more work items than threads (float32, from 4097 rows), and
# the last row count that fits. n gives several tiles with a ragged last one.
SHAPES = {
    ('float32', 'float32'): [(7, 70), (176, 70), (177, 70), (256, 70), (257, 70), (320, 70), (321, 70), (541, 40),
                             (1669, 20), (2049, 11), (3490, 7), (4097, 7), (4265, 7), (4549, 5)],
    ('float64', 'float32'): [(176, 70), (177, 70), (272, 40), (499, 40), (853, 11), (1370, 11), (2049, 7), (2408, 5)],
    ('float64', 'float64'): [(64, 70), (271, 40), (492, 40), (835, 11), (1365, 11), (2049, 7), (2274, 5)],
}
# the emulated twins (one OS thread per work-item): one shape per row of the forward-variant table, and the limits
SHAPES_EMULATED = {
    ('float32', 'float32'): [(176, 70), (256, 70), (320, 70), (321, 70), (4549, 5)],
    ('float64', 'float32'): [(176, 70), (177, 70), (2408, 5)],
    ('float64', 'float64'): [(271, 40), (2274, 5)],
}
# `rounded`: shapes at which some step has no matching row while its forward argmin is >= n (the fall-back is the
# argmin taken modulo n); float64 data with float32 penalties never falls back at these sizes
ROUNDED_FALLBACK = {('float32', 'float32'): [(177, 70), (321, 70), (1669, 20)],
                    ('float64', 'float64'): [(271, 40), (2274, 5)]}
BATCH_SHAPE = {('float32', 'float32'): (257, 40), ('float64', 'float32'): (177, 40), ('float64', 'float64'): (271, 40)}


def case_id(combo, shape=None, kind=None):
    s = '%s-%s' % (combo[0][-2:], combo[1][-2:])
    if shape is not None:
        s += '-%dx%d' % shape
    return s + ('-' + kind if kind else '')


def tracking_cases(shapes):
    return [(c, s, k) for c in COMBOS for s in shapes[c] for k in KINDS]


# ---- inputs --------------------------------------------------------------------------------------
def make_case(kind, na, n, dtype, pdtype, seed=SEED):
    """`(E (na, n) in dtype, sc (na,) in pdtype, penalty)` of one kind.

    random : E = -log(U + 1e-7), log-spaced scales, penalty 2 -- one matching row per backward step.
    ties   : E from {0, 1, 2}, sc = arange(na) // 2 (neighbouring rows share a scale: P has zeros off the diagonal),
             penalty 1 -- sums are small integers, exact in every type. Rows 2k and 2k+1 have the same penalties, so
             they match together wherever their E agree: the odd row copies the even one with probability 1/2
             (independent draws agree with probability 1/3), which makes two thirds of the steps ties.
    flat   : E from {0, 1, 2}, sc = arange(na), penalty 0 -- every row whose E is its column's minimum matches. Two
             rows of each column, one in the lowest and one in the highest third, are set to 0, so that at least
             two rows match at every step at any row count (by construction, not by the luck of the draw).
    rounded: E = 1000 + 3 U, sc = linspace(0, .5, na), penalty 40 -- the sums round, `pe - E` is not the minimum
             that went in, and some steps have no matching row."""
    rng = np.random.default_rng([seed, KINDS.index(kind), na, n])
    if kind == 'random':
        E = -np.log(rng.random((na, n)) + 1e-7)
        sc, penalty = np.log(np.exp(np.linspace(-0.3, 6.2, na)).astype(pdtype)), 2.0
    elif kind == 'ties':
        E = rng.integers(0, 3, (na, n))
        half = na // 2
        same = rng.random((half, n)) < 0.5
        E[1:2 * half:2][same] = E[0:2 * half:2][same]
        sc, penalty = np.arange(na) // 2, 1.0
    elif kind == 'flat':
        E = rng.integers(0, 3, (na, n))
        third = max(na // 3, 1)
        cols = np.arange(n)
        E[rng.integers(0, third, n), cols] = 0
        E[rng.integers(na - third, na, n), cols] = 0
        sc, penalty = np.arange(na), 0.0
    elif kind == 'rounded':
        E = 1000 + 3 * rng.random((na, n))
        sc, penalty = np.linspace(0, .5, na), 40.0
    else:
        raise ValueError(kind)
    return (np.ascontiguousarray(E, dtype=dtype), np.ascontiguousarray(sc, dtype=pdtype), penalty)


def penalty_matrix(sc, penalty):
    """`penalty * np.subtract.outer(sc, sc)**2` in sc's type, as the reference forms it."""
    return np.asarray(penalty, dtype=sc.dtype) * np.subtract.outer(sc, sc)**2


def eps_of(pdtype):
    return np.asarray(np.finfo(pdtype).eps, dtype=pdtype)


_REFERENCES = {}


def reference(orc, kind, combo, shape):
    """(E, sc, penalty, eps, pe_ref, ridge_ref) of one case: computed once per process, shared, read-only."""
    key = (kind, combo, shape)
    if key not in _REFERENCES:
        E, sc, penalty = make_case(kind, shape[0], shape[1], *combo)
        eps = eps_of(combo[1])
        ridge, pe = orc.ridge_track(E, penalty_matrix(sc, penalty), eps)
        for a in (E, sc, pe, ridge):
            a.setflags(write=False)
        _REFERENCES[key] = (E, sc, penalty, eps, pe, ridge)
    return _REFERENCES[key]


def backward_hits(E, P, pe, ridge, eps):
    """For the backward steps t = 0 .. n-2 of a finished tracking (`ridge`: its result): the number of rows f with
    |pe[r, t+1] - E[r, t+1] - (pe[f, t] + P[r, f])| < eps, r = ridge[t+1], and whether they lie in more than one
    group of 64 rows (the kernel ballots 64 rows at a time)."""
    T = E.dtype.type
    na, n = E.shape
    count, spans = np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=bool)
    with np.errstate(invalid='ignore'):
        for t in range(n - 2, -1, -1):
            r = ridge[t + 1]
            val = pe[r, t + 1] - E[r, t + 1]
            hit = np.flatnonzero(np.abs(val - (pe[:, t] + P[r].astype(T))) < T(eps))
            count[t] = hit.size
            spans[t] = hit.size > 0 and hit[0] // 64 != hit[-1] // 64
    return count, spans


# ---- the NumPy statement of extract_ridges ------------------------------------------------------------
def extract_ridges_numpy(Tf, scales, penalty=2., n_ridges=1, bw=15, transform='cwt', neglog=None):
    """`extract_ridges` as plain NumPy, loop for loop: np.amin (which propagates NaN), np.argmin (first NaN, else
    first minimum), Python slices. Slow: for small transforms. Returns (indices, frequencies, energies).
    `neglog(energy, energy_max, eps)` optionally replaces `-log(energy / energy_max + eps)`, as in the oracle."""
    Tf = np.asarray(Tf)
    dt = np.float64 if Tf.dtype == np.complex128 else np.float32
    eps = eps_of(dt)
    scales = np.asarray(scales, dtype=dt)
    sc = (np.log(scales) if transform == 'cwt' else scales).squeeze()
    P = penalty_matrix(sc, penalty)
    energy = np.abs(Tf)**2
    na, n = Tf.shape
    idx = np.zeros((n, n_ridges), dtype=int)
    freq, en = np.zeros((n, n_ridges), dtype=dt), np.zeros((n, n_ridges), dtype=dt)
    with np.errstate(all='ignore'):
        for i in range(n_ridges):
            energy_max = energy.max(axis=0)
            E = -np.log(energy / energy_max + eps) if neglog is None else neglog(energy, energy_max, eps)
            pe = E.copy()
            for t in range(1, n):
                for f in range(na):
                    pe[f, t] += np.amin(pe[:, t - 1] + P[f])
            ridge = np.unravel_index(np.argmin(pe, axis=0), pe.shape)[1]
            for t in range(n - 2, -1, -1):
                r = ridge[t + 1]
                val = pe[r, t + 1] - E[r, t + 1]
                for f in range(na):
                    if abs(val - (pe[f, t] + P[r, f])) < eps:
                        ridge[t] = f
            idx[:, i] = ridge
            freq[:, i] = scales.squeeze()[ridge]
            en[:, i] = energy[ridge, range(n)]
            for t in range(n):
                energy[int(ridge[t] - bw):int(ridge[t] + bw), t] = 0
    return idx, freq, en


def silent_transform(cdtype, where, na=40, n=30, seed=SEED):
    """A random complex (na, n) transform with all-zero columns `where` ('front' | 'middle' | 'end' | None)."""
    rng = np.random.default_rng([seed, na, n])
    Tf = ((rng.random((na, n)) + 0.1) * np.exp(2j * np.pi * rng.random((na, n)))).astype(cdtype)
    cols = {'front': [0, 1], 'middle': [n // 2, n // 2 + 1, n // 2 + 5], 'end': [n - 2, n - 1], None: []}[where]
    Tf[:, cols] = 0
    return Tf


# ---- comparisons over a driver ------------------------------------------------------------------------
# A driver runs the C entry points on NumPy arrays and returns NumPy arrays (on the GPU through device tensors, in the
# emulated twins on host memory):
#   drv.track(E, sc, penalty, eps, pe0=None, ridge0=None) -> (rc, pe, ridge); E (na, n) or (B, na, n) (the batch
#       entry point); pe0 / ridge0: what the output buffers hold before the call
#   drv.clear(en, ridge, bw, with_e) -> (rc, en, ridge_e or None); en (na, n) or (B, na, n)
#   drv.last_error() -> str
SENTINEL_PE, SENTINEL_RIDGE = -12345.5, -77


def check_tracking(drv, orc, kind, combo, shape):
    E, sc, penalty, eps, pe_ref, ridge_ref = reference(orc, kind, combo, shape)
    rc, pe, ridge = drv.track(E, sc, penalty, eps)
    assert rc == 0, drv.last_error()
    assert pe.dtype == pe_ref.dtype and np.array_equal(pe, pe_ref)
    assert np.array_equal(ridge, ridge_ref), np.flatnonzero(ridge != ridge_ref)


def check_tracking_batch(drv, orc, combo):
    shape = BATCH_SHAPE[combo]
    refs = [reference(orc, kind, combo, shape) for kind in ('flat', 'ties', 'rounded')]
    # one scale vector and penalty per call: each transform's own (E), tracked under the `ties` design
    sc, penalty, eps = refs[1][1], refs[1][2], refs[1][3]
    Eb = np.stack([r[0] for r in refs])
    rc, peb, rb = drv.track(Eb, sc, penalty, eps)
    assert rc == 0, drv.last_error()
    P = penalty_matrix(sc, penalty)
    for b in range(3):
        rc, pe1, r1 = drv.track(np.ascontiguousarray(Eb[b]), sc, penalty, eps)
        assert rc == 0, drv.last_error()
        assert np.array_equal(peb[b], pe1) and np.array_equal(rb[b], r1), b
        ridge_ref, pe_ref = orc.ridge_track(Eb[b], P, eps)
        assert np.array_equal(pe1, pe_ref) and np.array_equal(r1, ridge_ref), b


def check_refusal(drv, combo):
    """One row more than fits: refused before anything is launched -- the outputs keep what they held."""
    na, n = MAX_ROWS[combo] + 1, 3
    E, sc, penalty = make_case('ties', na, n, *combo)
    pe0 = np.full((na, n), SENTINEL_PE, dtype=combo[0])
    ridge0 = np.full(n, SENTINEL_RIDGE, dtype=np.int64)
    rc, pe, ridge = drv.track(E, sc, penalty, eps_of(combo[1]), pe0=pe0, ridge0=ridge0)
    assert rc != 0
    assert '%d rows' % na in drv.last_error(), drv.last_error()
    assert np.all(pe == SENTINEL_PE) and np.all(ridge == SENTINEL_RIDGE)
    # the library goes on working
    E, sc, penalty = make_case('ties', 65, 9, *combo)
    rc, pe, ridge = drv.track(E, sc, penalty, eps_of(combo[1]))
    assert rc == 0, drv.last_error()
    assert ridge.min() >= 0 and ridge.max() < 65


CLEAR_BW = (0, 0.5, 2.5, 4, 15, 'rows', '3rows')


def clear_reference(en, ridge, bw):
    """ref[int(r - bw):int(r + bw), t] = 0 per column; a ridge index outside [0, rows): column untouched, energy 0."""
    ref, na = en.copy(), en.shape[0]
    ridge_e = np.zeros(en.shape[1], dtype=en.dtype)
    for t, r in enumerate(ridge):
        if 0 <= r < na:
            ridge_e[t] = en[r, t]
            ref[int(r - bw):int(r + bw), t] = 0
    return ref, ridge_e


def check_clear(drv, dtype, na=37, n=70):
    rng = np.random.default_rng([SEED, na, n])
    B = 3
    enb = (rng.random((B, na, n)) + 0.5).astype(dtype)
    # 0, 1, rows - 1 and mid rows: the negative start wraps (int(r - bw) < 0 counts from the end), both ends clamp
    inside = np.resize(np.array([0, 1, na - 1, na // 2, 2, na - 2, na // 3, 5], dtype=np.int64), n)
    ridges = np.stack([inside, np.roll(inside, 3), rng.integers(0, na, n)])
    outside = inside.copy()
    outside[::7], outside[3::7] = -1, na            # the reference raises; the kernel leaves the column alone
    for bw in CLEAR_BW:
        bw = {'rows': na, '3rows': 3 * na}.get(bw, bw)
        for with_e in (True, False):
            for rv in (inside, outside):
                ref, e_ref = clear_reference(enb[0], rv, bw)
                rc, en, r_e = drv.clear(enb[0], rv, bw, with_e)
                assert rc == 0, drv.last_error()
                assert np.array_equal(en, ref), (bw, with_e)
                assert (r_e is None) if not with_e else np.array_equal(r_e, e_ref), (bw, with_e)
            rc, en, r_e = drv.clear(enb, ridges, bw, with_e)
            assert rc == 0, drv.last_error()
            for b in range(B):
                ref, e_ref = clear_reference(enb[b], ridges[b], bw)
                assert np.array_equal(en[b], ref), (bw, with_e, b)
                assert (r_e is None) if not with_e else np.array_equal(r_e[b], e_ref), (bw, with_e, b)
