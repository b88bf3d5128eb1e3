# -*- coding: utf-8 -*-
"""The host side of `reassign_cwt`: `wavelets.wavelet_time_std`, the per-row displacement bound,
the `C` and `sh` rule of the fixed-point sum, the default `home`, and the condition the kernel tests' equalities rest
on -- no committed seed has a point near a rounding boundary of the bin map or near `gamma`. CPU-only."""
import numpy as np
import pytest
import reassign2d as R
import reassign_cwt as Q

# the library's sizes (ssq_reassign_cwt_tile), restated: tests/test_gpu_reassign_cwt.py asserts the shapes against the
# library in use
TILE = (8, 256, 4, 64, 4096, 16, 384)


def test_names_are_exported_lazily():
    import ssqueezepy_amd
    from ssqueezepy_amd import _lib
    assert _lib.ABI_VERSION >= 117 and {'ssq_reassign_cwt', 'ssq_reassign_cwt_tile'} <= set(_lib.EXPORTS)
    for name in ('reassign_cwt', 'reassign_cwt_gpu', 'wavelet_time_std'):
        assert callable(getattr(ssqueezepy_amd, name))


def test_time_std_of_a_morlet_wavelet_is_sqrt_half():
    """``psih = exp(-(w - mu)^2 / 2)``: ``|psih'|^2 = (w - mu)^2 |psih|^2``, the variance of a Gaussian of variance 1/2."""
    from ssqueezepy_amd import Wavelet, wavelet_time_std
    for mu in (13.4, 10., 20.):               # (the library's Morlet has a correction term of relative size exp(-mu^2 / 2))
        for dtype in ('float32', 'float64'):
            got = wavelet_time_std(Wavelet(('morlet', {'mu': mu, 'dtype': dtype})))
            assert abs(got - np.sqrt(.5)) <= 1e-12 * np.sqrt(.5), (mu, dtype, got)
    assert wavelet_time_std(('morlet', {'mu': 13.4})) == wavelet_time_std(Wavelet(('morlet', {'mu': 13.4})))


@pytest.mark.parametrize('norm', ['bandpass', 'energy'])
def test_time_std_of_a_gmw_against_the_sampled_wavelet(norm):
    """GMW (3, 60): the second moment of ``|psi(t)|^2`` from the wavelet sampled in time -- an inverse FFT of `psih` on a
    grid fine and long enough for both ends -- over its zeroth (the first is 0: `psih` is real). Relative 1e-6."""
    from ssqueezepy_amd import Wavelet, wavelet_time_std
    wav = Wavelet(('gmw', {'gamma': 3, 'beta': 60, 'norm': norm, 'dtype': 'float64'}))
    M, scale = 1 << 16, 64.                       # the wavelet at scale 64: 3.5 x 64 samples of standard deviation in 65536
    k = np.arange(M)
    xi = np.where(k <= M // 2, k, k - M) * (2 * np.pi / M)
    psi = np.fft.ifft(np.asarray(wav.fn(scale * xi), dtype=np.float64))
    t = np.where(k <= M // 2, k, k - M).astype(np.float64)
    p = np.abs(psi) ** 2
    assert abs((t * p).sum() / p.sum()) < 1e-6
    want = np.sqrt((t * t * p).sum() / p.sum()) / scale
    got = wavelet_time_std(wav)
    assert abs(got - want) <= 1e-6 * want, (got, want)
    assert 3. < got < 4.


def test_time_std_refuses_what_derived_wavelets_refuses():
    from ssqueezepy_amd import Wavelet, wavelet_time_std
    for wavelet in ('bump', ('gmw', {'order': 1})):
        with pytest.raises(NotImplementedError):
            wavelet_time_std(Wavelet(wavelet))


def test_dmax_rule_on_its_edge_values():
    from ssqueezepy_amd import algos
    cap = algos.TSSQ_MAX_DMAX
    assert cap == Q.MAX_DMAX
    sc = np.array([.25, 1., 1. + 1e-12, 2., 1e5, cap / 2., cap / 2. + .25, 1e9])
    got = algos.reassign_cwt_dmax(sc, .5, 4.)                          # max_shift time_std = 2
    assert got.dtype == np.int32
    assert got.tolist() == [1, 2, 3, 4, 200000, cap, cap, cap]         # an integer product stays, anything above it goes up
    assert algos.reassign_cwt_dmax(sc, .5, 0.).tolist() == [0] * len(sc)
    assert algos.reassign_cwt_dmax([3.], np.sqrt(.5), 4.).tolist() == [int(np.ceil(4 * np.sqrt(.5) * 3))]
    for bad in (dict(max_shift=-1.), dict(max_shift=np.nan), dict(time_std=np.inf), dict(time_std=-.5)):
        kw = dict(dict(time_std=.5, max_shift=4.), **bad)
        with pytest.raises(ValueError):
            algos.reassign_cwt_dmax(sc, **kw)


def test_cell_terms_and_shift_at_bit_length_boundaries():
    """``C = sum_i min(2 dmax[i] + 1, n)`` with the frequency axis on, ``max_i`` with it off; ``sh = 62 - bit_length(C) -
    frexp(peak)[1]``: one more term at a power of two costs a bit, and ``C q`` stays below 2^62 for the largest term."""
    dmax = np.array([0, 1, 3, 1000])
    assert Q.cell_terms(dmax, 100, True) == 1 + 3 + 7 + 100 and Q.cell_terms(dmax, 100, False) == 100
    assert Q.cell_terms(dmax, 5, True) == 1 + 3 + 5 + 5 and Q.cell_terms(dmax, 5, False) == 5
    assert Q.cell_terms(dmax, 100, True, time=False) == 4 and Q.cell_terms(dmax, 100, False, time=False) == 1
    for C, H in ((1, 1), (2, 2), (3, 2), (4, 3), (255, 8), (256, 9), ((1 << 40) - 1, 40)):
        assert int(C).bit_length() == H
        for emax, ex in ((1., 1), (.5, 0), (.75, 0), (np.nextafter(1., 0.), 0), (3e-9, -28), (1e300, 997)):
            sh = R.shift(emax, C)
            assert sh == 62 - H - ex
            if -1000 < sh < 1000:
                q = int(np.ldexp(np.float64(emax), sh).astype(np.uint64))
                assert C * q < 2 ** 62 and 2 * (C + 1) * (q + 1) > 2 ** 60
    # rows of dmax = 0 and one column: C = rows with the frequency axis on
    assert Q.cell_terms(np.zeros(7, dtype=int), 1, True) == 7 and Q.cell_terms(np.zeros(7, dtype=int), 1, False) == 1


@pytest.mark.parametrize('idx', range(len(Q.SHAPE_IDS)), ids=Q.SHAPE_IDS)
def test_committed_seeds_have_no_point_near_a_boundary(idx):
    """For the shape's committed seed: no kept point within `NEAR_BOUNDARY` of a rounding boundary of the bin map and none
    within 1e-6 of `gamma`, on every grid, in both dtypes; and the seed is the smallest such."""
    shape = Q.shapes(*TILE)[idx]

    def clean(seed):
        for dtype in ('float32', 'float64'):
            W, dW, Wd, cst, rsc, dmax = Q.planes(shape, dtype, seed)
            gamma = R.quiet_gamma(W)
            if R.near_gamma(W, gamma).any():
                return False
            for kind in Q.GRIDS:
                near = Q.terms(W, dW, None, cst, rsc, dmax, Q.C.ssq_freqs(kind, shape[1]), gamma)[5]
                if near.any():
                    return False
        return True
    seed = Q.SEEDS.get(tuple(shape), 0)
    assert clean(seed)
    assert not any(clean(s) for s in range(seed))


def test_planes_are_what_the_cases_need():
    shape = (2, 9, 296, 64)
    W, dW, Wd, cst, rsc, dmax = Q.planes(shape, 'float64')
    assert dmax[0] == 0 and dmax[-1] == 64 and (np.diff(dmax[1:]) >= 0).all() and dmax.dtype == np.int32
    assert np.allclose(rsc[1:] / dmax[1:], 3.) and (cst >= .5).all() and (cst <= 2.).all()
    assert 500. < np.abs(W[1]).mean() / np.abs(W[0]).mean() < 2000.
    lands, k2, c2, ew, kept, _ = Q.terms(W, dW, Wd, cst, rsc, dmax, Q.C.ssq_freqs('log', 9), R.quiet_gamma(W))
    d = (c2 - np.arange(296)[None, None, :])[lands]
    assert d.min() == -64 and d.max() == 64 and .05 < kept.mean() - lands.mean() < .5      # both drop branches are taken
    assert (Q.row_dmax(5, 0) == 0).all() and Q.row_dmax(2, 4).tolist() == [1, 4]


@pytest.mark.parametrize('kind', Q.GRIDS)
def test_default_home_is_the_map_of_the_rows_own_frequencies(kind):
    """`algos.reassign_cwt_home` against `conceft_cwt.bins`, the NumPy statement of `bin_from_w`: the bin of ``wc fs / (2
    pi scales[i])``, mirrored by `flipud`; the rows themselves with the frequency axis off; without `wc`, the grid's top
    frequency stands for the smallest scale's."""
    from ssqueezepy_amd import algos
    rows = 40
    freqs = Q.C.ssq_freqs(kind, rows)
    sc = 2. ** np.linspace(-1., 5., rows)                # centre frequencies from beyond the grid's top to below its bottom
    wc, fs = 13.4, 20.
    fc = wc * fs / (2 * np.pi * sc)
    assert fc.max() > freqs.max() and fc.min() < freqs.min()
    kindp, p = Q.grid_params(freqs)
    k, near = Q.C.bins(fc, kindp, p, rows - 1)
    assert not near.any() and k[0] == rows - 1 and k[-1] == 0 and len(np.unique(k)) > rows // 2
    home = algos.reassign_cwt_home(sc, freqs, False, wc=wc, fs=fs)
    assert home.dtype == np.int32 and np.array_equal(home, k)
    assert np.array_equal(algos.reassign_cwt_home(sc, freqs, True, wc=wc, fs=fs), rows - 1 - k)
    assert np.array_equal(algos.reassign_cwt_home(sc, freqs, True, freq=False), np.arange(rows))
    k0, _ = Q.C.bins(freqs.max() * sc.min() / sc, kindp, p, rows - 1)
    assert np.array_equal(algos.reassign_cwt_home(sc, freqs), k0) and k0[0] == rows - 1


def test_restatement_orders_the_fm_tone():
    """The NumPy float64 restatement alone, through the library's design (Morlet, mu = 13.4, 32 voices, N = 4096, period
    300): the four shares are in strict order -- scalogram < min('freq', 'time'), max('freq', 'time') < 'both' -- and are
    the values DESIGN.md section 4.5.10 records."""
    s, f, t, b = Q.np_fm_shares(300.)
    assert s < min(f, t) and max(f, t) < b
    assert np.allclose([s, f, t, b], [0.3440, 0.6472, 0.5865, 0.9579], atol=5e-4)
