# -*- coding: utf-8 -*-
"""The routing rule of the reassignment kernels and the statements of tests/reassign_rows.py, on the host alone:
`ssq_reassign_route` (no device call) against `reassign_rows.route` -- the table restated from the LDS formulas -- for
every row count in 1 .. 7000, both data types, the three bin sources, ordered or not, with the bin map asked for or
not; the documented limits as numbers; `ordered_sum` against the oracle bit for bit; the spread condition of the
random inputs at every shape the GPU module uses; what the crafted planes are there for. CPU-only."""
import ctypes
import numpy as np
import pytest
import reassign_rows as R


@pytest.fixture(scope='module')
def A():
    from ssqueezepy_amd import algos, _lib
    _lib.load()
    return algos


def test_route_query_is_the_rule(A):
    n = 300
    seen = set()
    for dtype in ('float32', 'float64'):
        for src in R.BINSRCS:
            for ordered in (False, True):
                for kmap in (False, True):
                    for na in range(1, 7001):
                        want = R.route(dtype, src, na, n, ordered, kmap)
                        assert R.query(A, dtype, src, na, n, ordered, kmap) == want, (dtype, src, na, ordered, kmap)
                        seen.add((dtype,) + want)
    # every build of the table is reached: nine ordered ones, five of the unordered float64 tile
    assert {s for s in seen if s[1] != 'f64'} == set(R.BUILDS)
    assert {(s[0], s[2]) for s in seen if s[1] == 'f64'} == set(R.F64_BUILDS)


def test_route_of_2_pow_31_points_and_more(A):
    """The arms only ``na * n >= 2^31`` reaches: the one-wavefront tile of 16 columns, of 8 at half the LDS, and no
    unordered float64 tile. (No test launches them: tens of GB per case.)"""
    for dtype, nas in (('float32', (100, 640, 641, 1280, 1281, 2561, 5121)), ('float64', (100, 320, 321, 640, 641, 2561))):
        for na in nas:
            n = -(-2 ** 31 // na)
            for src in R.BINSRCS:
                want = R.route(dtype, src, na, n)
                assert want[0] in ('tile', 'global') and R.query(A, dtype, src, na, n) == want, (dtype, na, src)
                assert R.query(A, dtype, src, na, n - 1)[0] in ('tile16', 'f64') or na > R.ORDERED_LIMITS[dtype][-3]
    assert R.query(A, 'float32', 'dwx', 640, 2 ** 31 // 640 + 1) == ('tile', 16, 1)
    assert R.query(A, 'float32', 'dwx', 641, 2 ** 31 // 641 + 1) == ('tile', 8, 1)
    assert R.query(A, 'float32', 'dwx', 1281, 2 ** 31 // 1281 + 1) == ('tile', 8, 1)
    assert R.query(A, 'float64', 'bins', 320, 2 ** 31 // 320 + 1) == ('tile', 16, 1)


def test_route_query_refuses(A):
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    k, c, w = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    for args in ((5, 0, 10, 10), (0, 3, 10, 10), (0, -1, 10, 10), (0, 0, 0, 10), (1, 1, 10, 0), (1, 2, 65535, 10)):
        assert lib.ssq_reassign_route(*args, 0, 0, ctypes.byref(k), ctypes.byref(c), ctypes.byref(w)) == -1, args
        assert (k.value, c.value, w.value) == (-1, 0, 0)
    assert lib.ssq_reassign_route(1, 2, 65534, 10, 0, 0, None, None, None) == 0        # null outputs are allowed
    assert lib.ssq_reassign_route(1, 1, 65535, 10, 0, 0, ctypes.byref(k), None, None) == 0 and k.value == 3


def test_limits_are_the_documented_ones(A):
    """320, 1280, 2560, 5120 (float32); 640, 1280, 2560 (float64); 160, 640, 1280 (the unordered float64 tile): the row
    counts after which the route changes, from the rule and from the library."""
    for fn in (lambda *a: R.route(*a), lambda *a: R.query(A, *a)):
        for dtype in ('float32', 'float64'):
            edges = [na for na in range(1, 7000) if fn(dtype, 'dwx', na, 300) != fn(dtype, 'dwx', na + 1, 300)]
            assert tuple(edges) == R.ORDERED_LIMITS[dtype], (dtype, edges)
            assert edges == [na for na in range(1, 7000) if fn(dtype, 'w', na, 300) != fn(dtype, 'w', na + 1, 300)]
            f64 = [na for na in range(1, 7000)
                   if fn(dtype, 'bins', na, 300)[0] == 'f64' and fn(dtype, 'bins', na, 300) != fn(dtype, 'bins', na + 1, 300)]
            assert tuple(f64) == R.F64_LIMITS[dtype], (dtype, f64)
            # above the unordered tile, ordered, or with the bin map asked for: the ordered rows of the table
            for na in (1, 160, 161, 640, 641, 1280, 1281, 2561, 5121):
                assert fn(dtype, 'bins', na, 300, True) == fn(dtype, 'bins', na, 300, False, True) == fn(dtype, 'dwx', na, 300)
                if na > R.F64_LIMITS[dtype][-1]:
                    assert fn(dtype, 'bins', na, 300) == fn(dtype, 'dwx', na, 300)
    assert R.ORDERED_LIMITS == {'float32': (320, 1280, 2560, 5120), 'float64': (640, 1280, 2560)}
    assert R.F64_LIMITS == {'float32': (160, 640), 'float64': (160, 640, 1280)}
    for (dtype, kernel, cols, waves), (lo, hi) in R.BUILDS.items():
        assert R.route(dtype, 'dwx', lo, 300) == (kernel, cols, waves) == R.route(dtype, 'w', hi or 7000, 300)
    for (dtype, cols), (lo, hi) in R.F64_BUILDS.items():
        assert R.route(dtype, 'bins', lo, 300) == ('f64', cols, 8) == R.route(dtype, 'bins', hi, 300)
    # the row counts of the GPU module sit on both sides of every edge
    for dtype in ('float32', 'float64'):
        for e in R.ORDERED_LIMITS[dtype]:
            assert e in R.NAS[dtype] and e + 1 in R.NAS[dtype]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_ordered_sum_is_the_oracle(orc, dtype):
    for na, n, grid in ((37, 21, 'log'), (100, 40, 'linear'), (64, 33, 'log-piecewise')):
        c = R.spread_case(dtype, na, n, grid, seed=3)
        p = R.grid_params(c['sf'], grid)
        w = R.w_plane(orc, c)
        for kind in R.WEIGHTS:
            const = R.weight(kind, na, dtype)
            for flipud in (False, True):
                ref, k = orc.ssqueeze(c['Wx'], c['dWx'], grid, p, const, c['gamma'], flipud, typing=0, get_k=True)
                assert np.array_equal(R.ordered_sum(c['Wx'], k, const), ref), (na, grid, kind, flipud)
                assert (k < 0).sum() >= 6
            # a stored w: the bins of its finite points are the fused ones (same oracle arithmetic), inf = skip
            ref = orc.indexed_sum(c['Wx'], w, grid, p, const, True, typing=0)
            _, k = orc.ssqueeze(c['Wx'], c['dWx'], grid, p, const, c['gamma'], True, typing=0, get_k=True)
            kw = np.where(np.isinf(w), -1, k)
            assert np.array_equal(R.ordered_sum(c['Wx'], kw, const), ref), (na, grid, kind)


def test_exact_sum_agrees_with_fsum():
    import math
    Wx = R.wide_plane('float64', 40, 3)
    k = R.patterns(40, 3)['mod3']
    w = R.weight('vec64', 40, 'float64')
    m, S, Ab = R.exact_sum(Wx, k, w)
    for cell in range(3):
        terms = [float(Wx[i, 1].real) * float(w[i]) for i in range(40) if k[i, 1] == cell]
        assert m[cell, 1] == len(terms)
        assert abs(float(S[0][cell, 1]) - math.fsum(terms)) <= 2.0 ** -52 * abs(math.fsum(terms))
        assert abs(float(Ab[0][cell, 1]) - math.fsum(map(abs, terms))) <= 2.0 ** -52 * float(Ab[0][cell, 1])
    assert m[3:].sum() == 0 and not S[0][3:].any()


def test_spread_condition_at_every_shape(orc):
    """On the oracle's own bin map: at least 90 % of the bins receive a point and no bin holds more than 10 % of the
    points (`spread_bound`: what fewer than 18 rows allow). Two rows: the linear grid only -- two values are evenly
    spaced in any metric and no log grid is made of them."""
    for dtype in ('float32', 'float64'):
        for na in R.NAS[dtype]:
            n = R.columns_for(na)
            for grid in R.GRIDS if na > 2 else ('linear',):
                c = R.spread_case(dtype, na, n, grid)
                _, k = orc.ssqueeze(c['Wx'], c['dWx'], grid, R.grid_params(c['sf'], grid), 1., c['gamma'], False,
                                    typing=0, get_k=True)
                hit, top = R.spread_ok(k, na)
                assert hit >= 0.9 and top <= R.spread_bound(na), (dtype, na, grid, hit, top)
                assert (k == 0).sum() >= 0.03 * k.size and (k == na - 1).sum() >= 0.03 * k.size      # both clamps are hit
                assert (k < 0).sum() >= 5
                assert (c['Wx'] == 0).sum() == 1 and (c['dWx'] == 0).sum() >= 1
            if na > 2:
                c = R.spread_case(dtype, na, n, 'linear', stft=True)
                _, k = orc.ssqueeze(c['Wx'], c['dWx'], 'linear', R.grid_params(c['sf'], 'linear'), 1., c['gamma'], False,
                                    Sfs=c['Sfs'], typing=0, get_k=True)
                hit, top = R.spread_ok(k, na)
                assert hit >= 0.9 and top <= R.spread_bound(na), (dtype, na, 'stft', hit, top)
    assert abs(R.spread_bound(18) - 0.15) < 1e-12 and R.spread_bound(36) == 0.10 == R.spread_bound(5121)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_crafted_planes_do_what_they_are_for(orc, dtype):
    """Integer planes sum exactly in any order; wide planes depend on the order; the crafted maps, sent as a `w` plane or
    as a `dWx` on the linear grid, come back from the oracle as the same bins."""
    na, n = 203, 9
    P = R.patterns(na, n)
    assert set(P) == set(R.PATTERN_NAMES)
    Wi, wi = R.int_plane(dtype, na, n)
    Ww = R.wide_plane(dtype, na, n)
    differ = set()
    for name, k in P.items():
        fwd = R.ordered_sum(Wi, k, wi)
        rev = R.ordered_sum(Wi[::-1], k[::-1], wi[::-1])
        assert np.array_equal(fwd, rev), name
        m, S, Ab = R.exact_sum(Wi, k, wi)
        assert np.array_equal(fwd.real, S[0].astype(dtype)) and np.array_equal(fwd.imag, S[1].astype(dtype)), name
        c = R.weight('vec64', na, dtype)
        if not np.array_equal(R.ordered_sum(Ww, k, c), R.ordered_sum(Ww[::-1], k[::-1], c[::-1])):
            differ.add(name)
    assert differ >= set(P) - set(R.ORDER_FREE), differ
    sf = R.make_ssq_freqs(na, 'linear')
    p = R.grid_params(sf, 'linear')
    for name, k in P.items():
        w, dWx, Wx = R.pattern_planes(Ww, k, sf)
        _, kd = orc.ssqueeze(Wx, dWx, 'linear', p, 1., R.PATTERN_GAMMA, False, typing=0, get_k=True)
        assert np.array_equal(kd, k), name
        ref = orc.indexed_sum(Wx, w, 'linear', p, 1., False, typing=0)
        assert np.array_equal(ref, R.ordered_sum(Wx, k, 1.)), name
