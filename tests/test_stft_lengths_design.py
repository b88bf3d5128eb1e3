# -*- coding: utf-8 -*-
"""The planning rule of the mixed-radix STFT kernel and the table of tests/stft_lengths.py, on the host alone:
`ssq_stft_generic_shape` (no device call) against a Python restatement of the rule for every n_fft in 2 .. 5100, the
table's radices and G against both, and that the table holds what it is there for -- every radix in every position it
can take, both sides of every G edge, the full epilogues. CPU-only."""
import numpy as np
import pytest
import stft_lengths as L

ODD = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31)


@pytest.fixture(scope='module')
def lib():
    from ssqueezepy_amd import _lib
    return _lib.load()


def test_generic_shape_is_the_planning_rule(lib):
    took = 0
    for n in range(2, 5101):
        want = L.plan_rule(n)
        if n in L.POW2:                              # stft_fused_kernel's: the plan never asks for these
            assert want is not None and L.query(lib, n) is None
            continue
        assert L.query(lib, n) == want, n
        took += want is not None
        if want:
            radix, G = want
            assert int(np.prod(radix)) == n and 16 * n * G <= L.GEN_LDS_BYTES
            assert L.epilogue_points(n, G) <= L.GEN_MAX_EPI
    assert took > 600
    for n in (0, 1, -6, 65536, 3 ** 11, 1 << 40):
        assert L.query(lib, n) is None
    # null outputs are allowed: the answer alone
    assert lib.ssq_stft_generic_shape(598, None, None, None) == 1 and lib.ssq_stft_generic_shape(97, None, None, None) == 0


def test_g_edges_are_the_documented_ones():
    """G = 16 up to 156, 8 up to 312, 4 up to 1248, 2 up to 2496, 1 up to 4992, from the LDS formula."""
    def g_of(n):                                     # (without the factor rule: any n)
        G = 16
        while G > 4 and 16 * n * G > L.GEN_LDS_BYTES // 2:
            G //= 2
        while G > 1 and 16 * n * G > L.GEN_LDS_BYTES:
            G //= 2
        return G if 16 * n <= L.GEN_LDS_BYTES else 0
    edges = [n for n in range(2, 5100) if g_of(n) != g_of(n + 1)]
    assert edges == [156, 312, 1248, 2496, 4992] and [g_of(n) for n in edges] == [16, 8, 4, 2, 1]
    for (lo, hi), G in zip(L.G_EDGES, (16, 8, 4, 2, 1)):
        assert L.LENGTHS[lo].G == G and L.LENGTHS[hi].G == (G // 2 or None)
        # ... and no length the kernel takes lies between the two
        assert all(L.plan_rule(n) is None for n in range(lo + 1, hi))
    for n in L.FULL_EPILOGUE:
        assert L.epilogue_points(n, L.LENGTHS[n].G) == L.GEN_MAX_EPI


def test_table_matches_the_rule_and_the_library(lib):
    for n, e in L.LENGTHS.items():
        want = L.plan_rule(n)
        assert (want is None) == (e.radix is None), n
        assert e.why
        if want:
            assert (e.radix, e.G) == want == L.query(lib, n), n
            assert L.expected_algo(n) == 'fused-mixed-radix'
        else:
            assert L.expected_algo(n) == 'rocfft' and L.query(lib, n) is None
    assert all(L.expected_algo(n) == 'fused' for n in L.POW2)
    assert set(L.EMULATED) <= set(L.LENGTHS)


def test_table_covers_every_position():
    fused = {n: e.radix for n, e in L.LENGTHS.items() if e.radix}
    alone = {r[0] for r in fused.values() if len(r) == 1}
    first = {r[0] for r in fused.values() if len(r) > 1}
    last = {r[-1] for r in fused.values() if len(r) > 1}
    middle = {q for r in fused.values() for q in r[1:-1]}
    assert alone == {2, 3, 4, 5, 7, 8, 11, 13, 16, 17, 19, 23, 29, 31}
    assert first >= set(ODD) | {2, 4, 8, 16}
    assert last >= set(ODD) | {2, 4, 16}             # (8 is never last: 16s, 8s, 4s, a 2, and 8 x 2 = 16)
    assert middle >= set(ODD) | {2, 4, 8, 16}
    assert (31, 31) in fused.values()
    assert {e.G for e in L.LENGTHS.values() if e.radix} == {16, 8, 4, 2, 1}
    assert max(len(r) for r in fused.values()) == 8
    for n in (4998, 5000, 97, 74):
        assert L.LENGTHS[n].radix is None
    # the issue's lists
    for n in (93, 155, 217, 341, 403, 527, 589, 713, 899, 961, 9, 15, 21, 33, 39, 51, 57, 69, 87, 186, 310, 434, 682,
              806, 1054, 1178, 1426, 1798, 1922, 32, 64, 384, 96, 4096, 3072, 20, 40, 4374, 2187):
        assert n in fused, n


def test_shapes_leave_a_partial_last_group():
    for n, e in list(L.LENGTHS.items()) + [(n, L.Entry((), G, '')) for n, G in L.POW2.items()]:
        G = e.G or 1
        a, b = L.shapes(n, e.G)
        assert a['n_hops'] % G == (1 if G > 1 else 0) and a['n_hops'] == (a['N'] - 1) // a['hop'] + 1
        assert a['N'] > n // 2                        # (reflect padding of n // 2 samples)
        assert b['n_hops'] == b['N'] == 2 * G + 3 and b['hop'] == 1


@pytest.mark.parametrize('padtype', ['reflect', 'zero', 'symmetric', 'replicate', 'wrap'])
def test_pad_sources_restate_the_plans_rule(padtype):
    import ssqueezepy_amd as S
    for N, n_fft in ((49, 2), (49, 3), (300, 156), (301, 31), (5, 4992), (6657, 4992), (40, 9)):
        if padtype == 'symmetric' and N < n_fft // 2:
            continue                                 # (the host's `padsignal` mirrors once, as the reference's does)
        assert np.array_equal(L.pad_sources(S, N, n_fft, padtype), L.pad_sources_numpy(N, n_fft, padtype)), (N, n_fft)


def test_statement_of_a_pure_tone():
    """The statement itself: a complex exponential's bin through a rectangular window, not modulated, no padding
    effect on an interior frame."""
    n_fft, hop, N = 20, 3, 200
    x = np.cos(2 * np.pi * 4 * np.arange(N) / n_fft).astype(np.float32)
    win = np.ones(n_fft, np.float32)
    dwin = np.arange(n_fft, dtype=np.float32)
    src = L.pad_sources_numpy(N, n_fft, 'zero')
    r = L.statement(x, win, dwin, n_fft, hop, src, False)
    assert r['Sx'].shape == (n_fft // 2 + 1, (N - 1) // hop + 1) == r['dSx'].shape and r['znorm'].shape == (r['Sx'].shape[1],)
    c = 30                                           # an interior frame
    assert abs(abs(r['Sx'][4, c]) - n_fft / 2) < 1e-4 and np.abs(np.delete(r['Sx'][:, c], 4)).max() < 1e-4
    fr = x[c * hop - 10: c * hop + 10].astype(np.float64)
    assert np.allclose(r['dSx'][:, c], np.fft.rfft(fr * dwin)) and np.isclose(r['znorm'][c] ** 2, (fr**2 * (1 + dwin**2)).sum())
    # modulated: the rotation is ifftshift
    rm = L.statement(x, win, dwin, n_fft, hop, src, True)
    assert np.allclose(rm['dSx'][:, c], np.fft.rfft(np.fft.ifftshift(fr) * dwin))
    # the error measure: one ulp-sized slip in one column shows in that column alone
    out = r['Sx'].astype(np.complex64)
    e0 = L.column_errors(out, r['Sx'], r['znorm'])
    out[3, c] += np.complex64(100 * L.EPS32 * r['znorm'][c])
    e1 = L.column_errors(out, r['Sx'], r['znorm'])
    assert e0.max() < 1 and e1[c] > 90 and np.array_equal(np.delete(e0, c), np.delete(e1, c))
