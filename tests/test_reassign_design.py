# -*- coding: utf-8 -*-
"""The NumPy statement of `ssq_reassign2d` (tests/reassign2d.py) and the host side of `reassign2d_gpu` and
`reassign_stft`: what can be checked without the library. CPU-only."""
import numpy as np
import pytest
import reassign2d as R


@pytest.mark.parametrize('C', [1, 2, 3, 4, 255, 256, 257, 2 ** 40 - 1])
@pytest.mark.parametrize('emax', [1., .5, 2., 1.999999, 3e-320, 5e-324, 1.7e308, 2. ** -1022])
def test_shift_rule_on_edge_values(C, emax):
    """`C` terms of the peak itself stay below 2^62, and at least 2^60 where the peak is a normal number and `C` a
    power of two minus one or less than a bit short of it: ``sh`` neither overflows nor wastes a bit."""
    H = int(C).bit_length()
    assert 2 ** (H - 1) <= C < 2 ** H
    sh = R.shift(emax, C)
    q = int(np.ldexp(np.float64(emax), sh).astype(np.uint64))
    assert C * q < 2 ** 62
    assert q >= 2 ** (61 - H) and C * q >= 2 ** 60                  # f >= 1/2: the peak's term uses the top bit it may
    assert 2 ** (61 - H) <= q < 2 ** (62 - H)


def test_small_energies_truncate_to_zero():
    """An energy below ``2^-sh`` -- a denormal next to a peak of 1 -- is a term of 0, not a rounding to 1."""
    sh = R.shift(1., 1000)
    e = np.array([5e-324, 2. ** -sh * .999999, 2. ** -sh, 2. ** -sh * 1.5, 2. ** -sh * 1.999999, 1.])
    q = np.ldexp(e, sh).astype(np.uint64)
    assert q.tolist() == [0, 0, 1, 1, 1, 2 ** sh]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_fixed_point_sum_is_within_its_bound_of_a_float64_sum(dtype):
    """The statement's `Rx` lies below a float64 `np.add.at` of the same terms by at most (the cell's terms) x 2^-sh,
    plus the float64 sum's own rounding."""
    shape = (2, 9, 300, 64, 1, 2)
    Sx, dSx, Vtg = R.planes(shape, dtype)
    B, rows, n = Sx.shape
    ref = R.statement(Sx, dSx, Vtg, 2 * rows, R.FS, R.FS, 1, 64, 0.)
    lands, k2, c2, e, _ = R.terms(Sx, dSx, Vtg, 2 * rows, R.FS, R.FS, 1, 64, 0.)
    assert np.array_equal(lands, ref['lands'])
    for b in range(B):
        want, count = np.zeros(rows * n), np.zeros(rows * n)
        idx = (k2[b] * n + c2[b])[lands[b]]
        np.add.at(want, idx, e[b][lands[b]])
        np.add.at(count, idx, 1.)
        assert count.max() >= 4
        err = want - ref['Rx'][b].reshape(-1)
        bound = count * 2. ** -ref['sh'][b]
        slack = count * R.EPS['float64'] * want
        assert (err <= bound + slack).all() and (err >= -slack).all()
        assert bound.max() <= 1e-9 * want.max()
    assert ref['sh'][0] != ref['sh'][1]


def test_crafted_planes_give_their_displacements():
    for dtype in ('float32', 'float64'):
        rng = np.random.default_rng(1)
        m, d = rng.integers(-3, 4, (1, 6, 40)), rng.integers(-9, 10, (1, 6, 40))
        Sx, dSx, Vtg = R.crafted(1.5, m, d, dtype, 16)
        lands, k2, c2, e, kept = R.terms(Sx, dSx, Vtg, 16, R.FS, R.FS, 3, 9, 0.)
        k, c = np.arange(6)[None, :, None], np.arange(40)[None, None, :]
        assert kept.all() and (e == 2.25).all()
        assert np.array_equal(k2, np.abs(k + m)) and np.array_equal(c2, c + d)
        assert np.array_equal(lands, (np.abs(k + m) <= 5) & (c + d >= 0) & (c + d < 40))


@pytest.mark.parametrize('hop', [1, 8])
def test_numpy_restatement_of_the_fm_tone(hop):
    """The whole transform restated in NumPy float64 (`reassign2d.np_shares`) on the FM tone of the GPU test: the
    shares are strictly ordered, 'both' is above 0.9, and they are the product's figures (0.470 /
    0.569 / 0.951 / 0.998 at hop 1, 0.470 / 0.568 / 0.943 / 0.998 at hop 8) to 2e-3 -- the product's float32 and float64
    figures agree to four digits, so the restatement's may differ in the third by the window's derivative alone."""
    from conftest import report_measured
    got = R.np_shares(hop)
    want = {1: [.470, .569, .951, .998], 8: [.470, .568, .943, .998]}[hop]
    report_measured('reassign_numpy_fm_tone_hop%d' % hop, spectrogram=got[0], freq=got[1], time=got[2], both=got[3])
    assert got[0] < got[1] < got[2] < got[3] and got[3] > .9
    assert np.abs(np.array(got) - want).max() <= 2e-3


def test_abi_and_lazy_export():
    import ssqueezepy_amd
    from ssqueezepy_amd import _lib
    assert _lib.ABI_VERSION >= 115
    assert {'ssq_reassign2d', 'ssq_reassign2d_tile'} <= set(_lib.EXPORTS)
    assert ssqueezepy_amd.reassign_stft is ssqueezepy_amd._reassign_stft.reassign_stft
    assert ssqueezepy_amd.reassign2d_gpu is ssqueezepy_amd.algos.reassign2d_gpu


def test_host_side_refusals():
    from ssqueezepy_amd import algos
    with pytest.raises(ValueError, match='`gamma`'):
        algos.reassign2d_gpu(None, None, None, 8, 1, 1., None)
