# -*- coding: utf-8 -*-
"""The NumPy statement of `ssq_time_reassign` (tests/tssq.py) and the host side of `time_reassign_gpu` and
`tssq_stft`: the statement against a brute-force extended-precision evaluation, the exact rotation index, that
the order tests' planes can tell one order of additions from another, the defaults and the lazy export. No GPU.

The first four tests and the last check the oracle itself (tests/tssq.py), not the product: they are what entitles
the GPU and emulated tests to compare with `==`. The kernel's own index arithmetic is held to the statement in
`test_rotation_index_beyond_32_bits` of tests/test_gpu_tssq_stft.py and its emulated twin."""
import numpy as np
import pytest
from conftest import report_measured
import tssq
from tssq import FS


def brute_force(Sx, Vtg, rot, n_fft, hop, cps, dmax, gamma):
    """The definition point by point in `clongdouble`, Python integers for the indices. Returns `Tx` and the points
    whose displacement lies within 1e-9 of a half-integer or of `dmax` + 1/2 in extended precision (the float64
    statement may round those the other way)."""
    B, rows, n = Sx.shape
    Tx = np.zeros((B, rows, n), dtype=np.clongdouble)
    doubtful = np.zeros((B, rows, n), dtype=bool)
    for b in range(B):
        for i in range(rows):
            for c in range(n):
                g, t = np.clongdouble(Sx[b, i, c]), np.clongdouble(Vtg[b, i, c])
                if abs(g) < gamma:
                    continue
                sc = (t / g).real * np.longdouble(cps)
                doubtful[b, i, c] = abs(abs(sc - np.floor(sc)) - .5) < 1e-9
                d = int(np.rint(sc))
                c2 = c + d
                if abs(d) > dmax or c2 < 0 or c2 >= n:
                    continue
                Tx[b, i, c2] += g * np.clongdouble(rot[(i * c * hop) % n_fft])
    return Tx, doubtful


@pytest.mark.parametrize('shape', [(1, 2, 1, 4, 1, 2), (2, 5, 63, 8, 1, 4), (1, 3, 65, 16, 4, 2)], ids=tssq.shape_id)
def test_statement_vs_extended_precision(shape):
    """The smallest shape (and two more): the statement's float64 `Tx` against the brute-force evaluation, within
    ``4 n eps64 sum|Sx|`` per row -- a term's product and the row's additions round, nothing else differs."""
    B, rows, n, n_fft, hop, dmax = shape
    Sx, Vtg = tssq.planes(shape, 'float64')
    gamma = tssq.lower_quartile_gamma(Sx)
    rot = tssq.default_rot(n_fft)
    want, doubtful = brute_force(Sx, Vtg, rot, n_fft, hop, FS / hop, dmax, gamma)
    assert not doubtful.any()
    got = tssq.statement(Sx, Vtg, rot, n_fft, hop, FS / hop, dmax, gamma)
    assert np.array_equal(got != 0, want != 0)
    bound = 4 * n * tssq.EPS['float64'] * np.abs(Sx).sum(axis=-1, keepdims=True)
    err = np.abs(got - want.astype(np.complex128))
    report_measured('tssq_statement_%s' % tssq.shape_id(shape), max_err_over_bound=float((err / bound).max()))
    assert (err <= bound).all()


def test_rotation_index_is_exact_beyond_2_to_32():
    rng = np.random.default_rng(5)
    for n_fft, hop in [(1024, 1), (1000, 333), (2 ** 31 - 1, 2 ** 40 + 3), (4096, 4096), (7, 10 ** 12)]:
        i = rng.integers(0, min(n_fft, 2 ** 31), 200)
        c = rng.integers(2 ** 31, 2 ** 32, 200)
        got = tssq.rotation_index(i, c, hop, n_fft)
        want = [(int(a) * int(b) * hop) % n_fft for a, b in zip(i, c)]
        assert max(int(a) * int(b) * hop for a, b in zip(i, c)) > 2 ** 32
        assert got.tolist() == want, (n_fft, hop)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_conflict_planes_tell_the_order(dtype):
    """On the planes of the order tests the statement with its terms in descending `c` differs from the statement:
    a kernel that adds in another order cannot pass them by luck."""
    for name, (n, dmax, target) in tssq.conflict_cases(256).items():
        Sx = tssq.wide_range_plane(1, 3, n, dtype, 7, target)
        Vtg = tssq.to_targets(Sx, target)
        ok, c2, _, _ = tssq.terms(Sx, Vtg, None, 16, 1, FS, dmax, 0.)
        assert ok.all() and np.array_equal(c2, np.broadcast_to(target, c2.shape)), name
        a = tssq.statement(Sx, Vtg, None, 16, 1, FS, dmax, 0.)
        b = tssq.statement(Sx, Vtg, None, 16, 1, FS, dmax, 0., reverse=True)
        assert (a.astype(Sx.dtype) != b.astype(Sx.dtype)).any(), name


def test_default_dmax_and_rot(monkeypatch):
    import torch
    from ssqueezepy_amd import algos
    assert [algos.default_dmax(*a) for a in [(1024, 1), (128, 4), (129, 4), (100, 3), (128, 256), (1, 1)]] == \
        [512, 16, 16, 17, 1, 0]
    monkeypatch.setattr(algos, 'device', lambda: torch.device('cpu'))
    rot = algos.rotation_table(12)
    assert rot.dtype == torch.complex128 and np.array_equal(rot.numpy(), np.exp(-2j * np.pi * np.arange(12) / 12))
    assert algos.rotation_table(12) is rot and np.array_equal(rot.numpy(), tssq.default_rot(12))


def test_lazy_export():
    import ssqueezepy_amd
    from ssqueezepy_amd import _lib
    assert ssqueezepy_amd.tssq_stft is ssqueezepy_amd._tssq_stft.tssq_stft
    assert ssqueezepy_amd.time_reassign_gpu is ssqueezepy_amd.algos.time_reassign_gpu
    assert _lib.ABI_VERSION >= 113
    assert {'ssq_time_reassign', 'ssq_time_reassign_segment', 'ssq_time_reassign_max_dmax'} <= set(_lib.EXPORTS)


def test_numpy_restatement_on_the_impulse_and_the_pulse():
    """`tssq.np_tssq`, the float64 restatement the GPU test compares with: an impulse at 400 goes to its column
    entirely, and the dispersive pulse's +-1-column share is far above the plain STFT's."""
    x = np.zeros(1024)
    x[400] = 1.
    Tx, Sx = tssq.np_tssq(x, tssq.gauss_window(128), 1)
    E = np.abs(Tx) ** 2
    assert E[:, 400].sum() / E.sum() >= .9999
    coherent = np.abs(Sx).sum(axis=-1)
    assert (np.abs(np.abs(Tx[:, 400]) - coherent) <= 1e-12 * coherent).all()
    Tx, Sx = tssq.np_tssq(tssq.dispersive_pulse(), tssq.gauss_window(128), 1)
    share, plain = tssq.delay_share(Tx, 128, 1), tssq.delay_share(Sx, 128, 1)
    report_measured('tssq_numpy_dispersive_pulse', share=share, stft_share=plain)
    assert share > .9 and plain < .5 * share
