# -*- coding: utf-8 -*-
"""The device-table cache of `ssq_cwt2_phase` (the rows' ``scale / fs``) and `ssq_conceft` (the projections): a
table is uploaded once per (device, contents), the eight most recent stay and the oldest is freed. Nine different
tables pass through each entry, so the first is evicted; then the first (uploaded again) and the ninth (found)
are used once more. Every call must give the bits of the first call with its arguments."""
import numpy as np
import pytest
import conceft
from conceft import _np

pytestmark = pytest.mark.gpu
KEPT = 8                                    # tables the cache keeps
FS = 200.


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def cwt2_calls(S):
    """`call(t)`: the second-order CWT map of five seeded 5 x 7 planes with the t-th of nine scale vectors."""
    rng = np.random.default_rng(8)
    planes = [(rng.standard_normal((5, 7)) + 1j * rng.standard_normal((5, 7))).astype(np.complex128) for _ in range(5)]
    scales = [np.geomspace(2, 40, 5) * (1 + .1 * t) for t in range(KEPT + 1)]
    return lambda t: _np(S.phase_cwt2_gpu(*planes, scales[t], FS, .5, .5)).copy()


def conceft_calls(S):
    """`call(t)`: `ssq_conceft` on the smallest planes of tests/conceft.py with the t-th of nine projection sets
    (one unit projection of one plane: the complex average is the reassigned plane turned by it)."""
    V, dV, _, Sfs = conceft.planes(conceft.SHAPES[0], 'float64')
    gamma = conceft.above_median(np.abs(V))
    projs = [np.exp(1j * (.3 + .5 * t)).reshape(1, 1) for t in range(KEPT + 1)]
    return lambda t: _np(S.conceft_gpu(list(V), list(dV), Sfs, projs[t], Sfs, gamma, False, 'complex')).copy()


@pytest.mark.parametrize('entry', ['ssq_cwt2_phase', 'ssq_conceft'])
def test_more_tables_than_the_cache_keeps(S, entry):
    call = (cwt2_calls if entry == 'ssq_cwt2_phase' else conceft_calls)(S)
    first = [call(t) for t in range(KEPT + 1)]
    for t in range(1, KEPT + 1):            # the tables matter: a stale one would show
        assert np.isfinite(first[t]).any() and not np.array_equal(first[t], first[0]), t
    assert np.array_equal(call(0), first[0], equal_nan=True)            # evicted by the ninth: uploaded again
    assert np.array_equal(call(KEPT), first[KEPT], equal_nan=True)      # still there
