# -*- coding: utf-8 -*-
"""`morse_wavelets`: the orthogonal generalized Morse tapers of `conceft_cwt` (host NumPy), and the new public
names."""
import numpy as np
import pytest
from conftest import report_measured
import ssqueezepy_amd
from ssqueezepy_amd.wavelets import Wavelet, morse_wavelets

SCALE, POINTS, ORDERS, GAMMA = 4., 1 << 16, 6, 3.


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('beta', [5., 20., 60.])
def test_orders_norm_and_dtype_are_kept(beta, dtype):
    tapers = morse_wavelets(('gmw', dict(gamma=GAMMA, beta=beta, dtype=dtype)), 5)
    assert [w.config['order'] for w in tapers] == [0, 1, 2, 3, 4]
    for w in tapers:
        assert isinstance(w, Wavelet) and w.family == 'gmw' and w.dtype == dtype
        assert (w.config['gamma'], w.config['beta'], w.config['norm']) == (GAMMA, beta, 'bandpass')
    # a Wavelet of another order gives the same family, and an 'energy' GMW keeps its norm
    again = morse_wavelets(tapers[3], 5)
    assert [w.key() for w in again] == [w.key() for w in tapers]
    assert morse_wavelets(('gmw', dict(norm='energy')), 2)[1].config['norm'] == 'energy'


def gram(beta, dtype):
    """The Gram matrix of orders 0 .. 5 sampled at ``SCALE * w``, `POINTS` points of ``w`` in ``[0, pi)``: the
    diagonal's spread relative to its mean and the largest ``|G_jk| / sqrt(G_jj G_kk)``, ``j != k``. The samples are
    the wavelets' own, in their dtype; the sums are taken in float64."""
    tapers = morse_wavelets(('gmw', dict(gamma=GAMMA, beta=beta, dtype=dtype)), ORDERS)
    w = np.arange(POINTS) * (np.pi / POINTS)
    P = np.stack([np.asarray(wv(SCALE * w)) for wv in tapers])
    assert P.dtype == np.dtype(dtype)
    G = P.astype(np.float64) @ P.astype(np.float64).T
    d = np.diag(G)
    off = np.abs(G / np.sqrt(np.outer(d, d)) - np.eye(ORDERS)).max()
    return float((d.max() - d.min()) / d.mean()), float(off)


@pytest.mark.parametrize('dtype, bound', [('float64', 1e-8), ('float32', 1e-3)])
def test_tapers_are_orthogonal_with_equal_norms(dtype, bound):
    """Equal diagonal within 1e-4; normalised off-diagonal at most 1e-8 (float64) and 1e-3 (float32): about 70x and
    5x what was measured at beta = 60, the worst of the three -- 1.4e-10 and 1.8e-4 (beta = 20: 2.6e-12, 3.4e-5;
    beta = 5: 2.9e-14, 2.8e-6). The values of this run are recorded."""
    for beta in (5., 20., 60.):
        spread, off = gram(beta, dtype)
        report_measured('conceft_cwt_morse_gram_%s_beta%d' % (dtype, beta), diagonal_spread=spread, off_diagonal=off)
        assert spread <= 1e-4 and off <= bound, (beta, spread, off)


def test_refusals():
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match='n_tapers'):
            morse_wavelets('gmw', bad)
    for other in ('morlet', Wavelet('bump'), ('hhhat', {})):
        with pytest.raises(ValueError, match='must be a GMW'):
            morse_wavelets(other, 3)
    assert len(morse_wavelets('gmw', 1)) == 1 and len(morse_wavelets('gmw', 8)) == 8


def test_new_names_resolve_lazily():
    for name in ('conceft_cwt', 'morse_wavelets', 'conceft_cwt_gpu'):
        ssqueezepy_amd.__dict__.pop(name, None)
        assert callable(getattr(ssqueezepy_amd, name)) and name in ssqueezepy_amd.__dict__
    assert ssqueezepy_amd.morse_wavelets is morse_wavelets
    from ssqueezepy_amd import _lib
    assert _lib.ABI_VERSION >= 112 and 'ssq_conceft_cwt' in _lib.EXPORTS
