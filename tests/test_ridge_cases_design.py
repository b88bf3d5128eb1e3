# -*- coding: utf-8 -*-
"""The inputs of the ridge-tracking tests (tests/ridge_cases.py) exercise what they are for: checked with the CPU
oracle, so that a change to a generator, a seed or a shape list cannot quietly turn the tie, fall-back and span cases
of tests/test_gpu_ridge_shapes.py into single-match cases again. CPU-only."""
import os
import re
import numpy as np
import pytest
import ridge_cases as rc
from conftest import ROOT

ALL = [(c, s) for c in rc.COMBOS for s in rc.SHAPES[c]]
IDS = [rc.case_id(c, s) for c, s in ALL]


def _hits(orc, kind, combo, shape):
    E, sc, penalty, eps, pe, ridge = rc.reference(orc, kind, combo, shape)
    count, spans = rc.backward_hits(E, rc.penalty_matrix(sc, penalty), pe, ridge, eps)
    return count, spans, pe


@pytest.mark.parametrize('combo,shape', ALL, ids=IDS)
def test_flat_ties_at_every_step(orc, combo, shape):
    count, spans, _ = _hits(orc, 'flat', combo, shape)
    assert (count >= 2).all(), count
    if shape[0] >= 177:                    # three groups of 64 rows or more: the matches are in several of them
        assert spans.all(), spans


@pytest.mark.parametrize('combo,shape', ALL, ids=IDS)
def test_ties_tie_at_a_third_of_the_steps(orc, combo, shape):
    count, _, _ = _hits(orc, 'ties', combo, shape)
    assert 3 * (count >= 2).sum() >= count.size, (int((count >= 2).sum()), count.size)


@pytest.mark.parametrize('combo,shape', [(c, s) for c in rc.ROUNDED_FALLBACK for s in rc.ROUNDED_FALLBACK[c]],
                         ids=[rc.case_id(c, s) for c in rc.ROUNDED_FALLBACK for s in rc.ROUNDED_FALLBACK[c]])
def test_rounded_falls_back_to_a_wrapped_argmin(orc, combo, shape):
    """A step without a matching row keeps the forward result, `argmin % n`: here with argmin >= n."""
    assert shape in rc.SHAPES[combo]
    count, _, pe = _hits(orc, 'rounded', combo, shape)
    argmin = np.argmin(pe, axis=0)[:-1]
    assert ((count == 0) & (argmin >= shape[1])).any(), (count, argmin)


@pytest.mark.parametrize('combo,shape', ALL, ids=IDS)
def test_random_never_ties(orc, combo, shape):
    """Why the smooth random energies of tests/test_gpu_ridges.py are not enough on their own."""
    count, _, _ = _hits(orc, 'random', combo, shape)
    assert (count <= 1).all(), count


def test_emulated_shapes_are_a_subset():
    for combo in rc.COMBOS:
        assert set(rc.SHAPES_EMULATED[combo]) <= set(rc.SHAPES[combo])
        assert (rc.MAX_ROWS[combo], 5) in rc.SHAPES[combo] and (rc.MAX_ROWS[combo], 5) in rc.SHAPES_EMULATED[combo]


def test_limits_are_the_documented_ones():
    """MAX_ROWS quotes include/ssq_hip.h; the README states the same figures; and they are what the backward
    kernel's LDS layout gives (csrc/ssq_ridge.hip: two (rows, 1 + 3) tiles, rows + 2 scales, one index, 64 bytes
    of slack, in 160 KiB)."""
    with open(os.path.join(ROOT, 'include', 'ssq_hip.h')) as fh:
        header = re.sub(r'[\s*]+', ' ', fh.read())
    with open(os.path.join(ROOT, 'README.md')) as fh:
        readme = re.sub(r'\s+', ' ', fh.read())
    quote = ("at most %d rows of float32 data, %d rows of float64 data with float32 penalties, "
             "%d rows of float64 data with float64 penalties" % tuple(rc.MAX_ROWS[c] for c in rc.COMBOS))
    assert quote in header
    assert quote in readme
    for (dt, pdt), rows in rc.MAX_ROWS.items():
        lds = lambda na: 2 * na * 4 * np.dtype(dt).itemsize + (na + 2) * np.dtype(pdt).itemsize + 4 + 64
        assert lds(rows) <= 160 * 1024 < lds(rows + 1)
