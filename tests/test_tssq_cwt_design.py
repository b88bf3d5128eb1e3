# -*- coding: utf-8 -*-
"""The host side of `tssq_cwt`: the two-level rotation tables against exact rational
arithmetic, the `sh` rule of the signed fixed-point sum with the inequality its proof rests on, the tile query's
documented relations, and the condition the kernel tests' equalities rest on -- no committed case has a point near
`gamma`. CPU-only."""
from fractions import Fraction
import numpy as np
import pytest
import reassign2d as R
import tssq_cwt as Q

_TILE = []


def tile():
    """(tile rows, tile columns, halo columns, window columns, most workgroups, P) of the built library, asked on the host
    (no device needed), as tests/test_gpu_tssq_cwt.py asks the library in use."""
    if not _TILE:
        import ctypes
        from ssqueezepy_amd import build, _lib
        lib = ctypes.CDLL(build.build(verbose=False))
        lib.ssq_version.restype = ctypes.c_int
        assert lib.ssq_version() >= 120
        fn = lib.ssq_time_reassign_cwt_tile
        fn.restype, fn.argtypes = _lib._PROTOS['ssq_time_reassign_cwt_tile']
        _TILE.append((tuple(fn(i) for i in range(6)), fn))
    return _TILE[0]


def test_names_are_exported_lazily():
    import ssqueezepy_amd
    from ssqueezepy_amd import _lib
    assert _lib.ABI_VERSION >= 120 and {'ssq_time_reassign_cwt', 'ssq_time_reassign_cwt_tile'} <= set(_lib.EXPORTS)
    assert _lib.TSSQ_CWT_ROT_P == Q.P and _lib.TSSQ_CWT_NO_WINDOW == 1
    for name in ('tssq_cwt', 'time_reassign_cwt_gpu', 'cwt_rotation_tables'):
        assert callable(getattr(ssqueezepy_amd, name))


def test_tile_query_against_its_documented_relations():
    """The built library, asked on the host: the window is the tile plus the halo twice, a tile is `P` columns wide (so
    `rot_hi` is uniform over a tile's row) and as many rows as a workgroup of 512 takes in one pass, a line of the
    write-out's (rows, 2 n) view is a wavefront wide, and the window of 16-byte cells fits the LDS of a CU."""
    from ssqueezepy_amd import _lib
    (tr, tc, hc, wc, gcap, p), fn = tile()
    assert wc == tc + 2 * hc and p == tc == _lib.TSSQ_CWT_ROT_P == Q.P and (2 * wc) % 64 == 0
    assert tr * tc == 512 and hc >= 0 and gcap >= 1 and tr * wc * 16 <= 160 * 1024
    assert fn(6) == 0 and fn(-1) == 0


def exact_turn(phi, k):
    """``frac(phi k)`` as a Fraction, `phi` the float64 it is."""
    v = Fraction(float(phi)) * k
    return v - (v.numerator // v.denominator)


def test_rotation_tables_against_fraction_arithmetic():
    from ssqueezepy_amd import algos
    phi = np.array([.3137, 1. / 3., .45, .0200001, 2. ** -7])
    n = 160000
    lo, hi = Q.tables(phi, n)
    assert lo.shape == (5, Q.P) and hi.shape == (5, -(-n // Q.P)) and lo.dtype == hi.dtype == np.complex128
    turns_lo, turns_hi = algos._exact_turns(phi, 1, Q.P), algos._exact_turns(phi, Q.P, hi.shape[1])
    for i in range(len(phi)):
        for k in (0, 1, 2, 100, Q.P - 1):
            f = exact_turn(phi[i], k)
            assert turns_lo[i, k] == float(f) and 0 <= turns_lo[i, k] < 1
            assert lo[i, k] == np.exp(-2j * np.pi * float(f))
        for q in (0, 1, 7, hi.shape[1] - 1):
            f = exact_turn(phi[i], Q.P * q)
            assert turns_hi[i, q] == float(f)
            assert hi[i, q] == np.exp(-2j * np.pi * float(f))
    assert (lo[:, 0] == 1).all() and (hi[:, 0] == 1).all()
    assert (lo[4, :] == np.exp(-2j * np.pi * ((np.arange(Q.P) % 128) / 128.))).all()        # a dyadic frequency: exact turns


def test_two_level_product_against_the_exactly_reduced_value():
    """At n = 160 000: the product of the two entries is within a few ulp of ``exp(-2j pi frac(phi c))`` with the exact
    fractional part, at every column; a direct ``np.exp(-2j pi phi c)`` is off by orders of magnitude more."""
    phi = np.array([.3137, .0200001, .44999])
    n = 160000
    lo, hi = Q.tables(phi, n)
    c = np.arange(n)
    prod = hi[:, c // Q.P] * lo[:, c % Q.P]
    cols = np.unique(np.concatenate([np.arange(0, n, 997), [n - 1, Q.P - 1, Q.P, n - Q.P]]))
    worst = naive = 0.
    for i in range(len(phi)):
        want = np.array([np.exp(-2j * np.pi * float(exact_turn(phi[i], int(k)))) for k in cols])
        worst = max(worst, np.abs(prod[i, cols] - want).max())
        naive = max(naive, np.abs(np.exp(-2j * np.pi * phi[i] * cols) - want).max())
    print('two-level product off by %.2e, naive exp by %.2e' % (worst, naive))
    # two entries rounded to within an ulp of a unit-modulus value, the angle to half an ulp of a turn (2 pi x 1.1e-16),
    # and one complex product: 8 eps covers it
    assert worst <= 8 * R.EPS['float64'] and naive > 1e3 * worst


def test_shift_rule_on_its_edge_values_and_the_proof_inequality():
    """``sh = 61 - bit_length(C) - ceil(ex / 2)``: `ex` odd and even, negative and positive, `C` at a power of two and one
    below; and the inequality of the proof: `C` terms of magnitude ``sqrt(emax) (1 + 4 eps)`` stay below 2^62 -- while
    they pass 2^60 for an odd exponent with `C` just below a power of two, so no bit is wasted."""
    from ssqueezepy_amd import algos
    eps = R.EPS['float64']
    for C, H in ((1, 1), (2, 2), (3, 2), (4, 3), (255, 8), (256, 9), ((1 << 21) + 1, 22)):
        assert int(C).bit_length() == H
        for emax, ex in ((1., 1), (.5, 0), (.75, 0), (np.nextafter(1., 0.), 0), (2., 2), (3.9, 2), (4., 3), (.25, -1),
                         (.2, -2), (.125, -2), (3e-9, -28), (2. ** -31, -30), (1e300, 997), (1e-300, -996)):
            assert int(np.frexp(emax)[1]) == ex
            hx = -((-ex) // 2)
            assert hx in (ex / 2, (ex + 1) / 2)
            sh = Q.shift(emax, C)
            assert sh == 61 - H - hx
            # the product's own host form of the rule, for a row whose bound gives this C
            assert algos.time_reassign_cwt_shift(emax, [0, C // 2], C) == sh
            assert algos.time_reassign_cwt_shift(emax, [C, 1], C) == sh          # (the bound is clipped at n)
            top = np.sqrt(emax) * (1 + 4 * eps)
            assert top < 2. ** hx * (1 + 8 * eps)
            q = int(np.trunc(np.ldexp(top, sh)))
            assert C * q < 2 ** 62
            assert C * q <= 2 ** 61 * (1 + 2. ** -40)           # the sum's own bound: 2^61 and a few ulp
    assert 255 * int(np.ldexp(np.sqrt(np.nextafter(1., 0.)), Q.shift(np.nextafter(1., 0.), 255))) > 2 ** 60
    assert Q.cell_terms([0, 1, 3, 1000], 100) == 100 and Q.cell_terms([0, 1, 3], 100) == 7 and Q.cell_terms([0], 1) == 1


@pytest.mark.parametrize('idx', range(len(Q.SHAPE_IDS)), ids=Q.SHAPE_IDS)
def test_committed_cases_have_no_point_near_gamma(idx):
    """The shapes are the GPU module's, from the built library's sizes; next to the condition on `gamma`, the `sh` the
    statement takes for every signal is the one `algos.time_reassign_cwt_shift` gives."""
    from ssqueezepy_amd import algos
    sizes = tile()[0]
    shape = Q.shapes(*sizes)[idx]
    for dtype in ('float32', 'float64'):
        W, Wd, rsc, dmax, phi = Q.planes(shape, dtype, hc=sizes[2])
        gamma = R.quiet_gamma(W)
        assert not R.near_gamma(W, gamma).any()
        assert len(dmax) == shape[1] and (phi > 0).all() and (phi < .5).all()
        e, kept = R.energy(W, gamma)
        for b in range(shape[0]):
            assert kept[b].any()
            emax = e[b][kept[b]].max()
            assert algos.time_reassign_cwt_shift(emax, dmax, shape[2]) == Q.shift(emax, Q.cell_terms(dmax, shape[2]))


def test_restatement_sharpens_both_signals():
    """The NumPy float64 restatement alone (N = 512, as the emulated module runs it): the share of ``|Tx|^2`` at the true
    group delay is above the scalogram's for the impulse and for the dispersive pulse, and without the rotation the
    impulse's terms cancel."""
    for kind in ('impulse', 'dispersive'):
        got, scal = Q.np_shares(kind, 512)
        print('%s: restatement share %.6f, scalogram %.6f' % (kind, got, scal))
        assert got > scal and got > .5
    x, wavelet, rows, tg, half = Q.e2e_case('impulse', 512)
    wav, sc, freqs, dmax = Q.design(wavelet, 512)
    Tx, W = Q.np_tssq(x, wav, sc, freqs, dmax, 10 * R.EPS['float64'])
    Tn, _ = Q.np_tssq(x, wav, sc, 0 * freqs, dmax, 10 * R.EPS['float64'])
    # the restatement's direct `exp` of the reduced angle against the product of the library's two table entries
    lo, hi = Q.tables(freqs, 512)
    c = np.arange(512)
    direct = np.exp(-2j * np.pi * np.mod(freqs[:, None] * c[None, :], 1.))
    assert np.abs(hi[:, c // Q.P] * lo[:, c % Q.P] - direct).max() <= 512 * 8 * R.EPS['float64']
    n0 = int(tg[0])
    i = rows[len(rows) // 2]
    bound = np.abs(W[i]).sum()
    assert np.abs(Tx[i, n0 - 1:n0 + 2]).sum() > .9 * bound and np.abs(Tn[i, n0 - 1:n0 + 2]).sum() < .1 * bound
