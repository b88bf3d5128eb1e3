# -*- coding: utf-8 -*-
"""`wavelets.derived_wavelets`: the banks ``psih'(w)`` and ``w psih(w)`` that `ssq_cwt2` transforms with
(DESIGN.md section 4.5.4). CPU-only.

The closed-form derivative is compared with a float64 central difference of the family's own function,
``D_h = (psih(w + h) - psih(w - h)) / 2h`` at ``h = 1e-4``, on ``w in [0, 12]``, within 1e-6 of
``max |psih'|``. The difference is itself off by ``h^2 psih''' / 6`` (truncation) plus ``eps |psih| / h``
(rounding, ~1e-11 here). Each case shows that this is below the tolerance before it uses the difference:
``D_h - D_{h/2}`` is 3/4 of the truncation error of `D_h` to leading order, so ``4/3 max|D_h - D_{h/2}|``
estimates it, and that figure must be under the tolerance. It is not far under it (a tenth to two thirds), so
the closed form is also held against the Richardson combination ``(4 D_{h/2} - D_h) / 3``, whose truncation
is ``O(h^4)`` (~1e-15) and whose rounding error is ``5/3 * 2 u max|psih| / h`` with `u` the relative error
of `psih` itself -- `eps` for the Morlet, ~``beta eps`` for the GMW, which exponentiates a sum of terms of
size `beta` -- so 3e-11 to 1e-9: within 1e-8 of ``max |psih'|``."""
import numpy as np
import pytest

from ssqueezepy_amd.wavelets import Wavelet, derived_wavelets

H = 1e-4
W_AXIS = np.linspace(0, 12, 2401)
TOL = 1e-6

CASES = [('gmw', dict(gamma=3, beta=60, norm='bandpass')), ('gmw', dict(gamma=3, beta=60, norm='energy')),
         ('gmw', dict(gamma=3, beta=5, norm='bandpass')), ('gmw', dict(gamma=3, beta=5, norm='energy')),
         ('gmw', dict(gamma=3, beta=60, norm='bandpass', centered_scale=True)),
         ('morlet', dict(mu=6)), ('morlet', dict(mu=13.4))]


def _id(case):
    return case[0] + '-' + '-'.join('%s' % v for v in case[1].values())


def central_difference(fn, w, h):
    return (np.asarray(fn(w + h), dtype=np.float64) - np.asarray(fn(w - h), dtype=np.float64)) / (2 * h)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_derivative_vs_central_difference(case):
    name, opts = case
    wav = Wavelet((name, dict(opts, dtype='float64')))
    dwav, wwav = derived_wavelets(wav)
    assert dwav.dtype == wwav.dtype == wav.dtype == 'float64'
    closed = np.asarray(dwav.fn(W_AXIS.copy()))
    assert closed.dtype == np.float64 and closed.shape == W_AXIS.shape and np.isfinite(closed).all()
    d_h = central_difference(wav.fn, W_AXIS, H)
    d_h2 = central_difference(wav.fn, W_AXIS, H / 2)
    peak = np.abs(closed).max()
    assert peak > 0
    truncation = 4 / 3 * np.abs(d_h - d_h2).max()
    err = np.abs(closed - d_h).max()
    err_r = np.abs(closed - (4 * d_h2 - d_h) / 3).max()
    print("measured: %s  max|psih'| %.4g  truncation of D_h %.3g  |closed - D_h| %.3g  (tolerance %.3g)  "
          "|closed - Richardson| %.3g" % (_id(case), peak, truncation, err, TOL * peak, err_r))
    assert truncation <= TOL * peak, (truncation, peak)             # the yardstick is finer than the tolerance
    assert err <= TOL * peak, (err, peak)
    assert err_r <= 1e-8 * peak, (err_r, peak)
    # the second companion is the product itself
    assert np.array_equal(np.asarray(wwav.fn(W_AXIS.copy())), W_AXIS * np.asarray(wav.fn(W_AXIS.copy())))


@pytest.mark.parametrize('norm', ['bandpass', 'energy'])
@pytest.mark.parametrize('beta', [60, 5, .5])
@pytest.mark.parametrize('centered', [False, True])
def test_gmw_is_zero_at_and_below_zero(norm, beta, centered):
    wav = Wavelet(('gmw', dict(gamma=3, beta=beta, norm=norm, centered_scale=centered, dtype='float64')))
    w = np.array([-12., -1., -1e-300, -0., 0., 5e-324, 1e-200, .5])       # (w = 1 is the peak of a centered GMW)
    for d in derived_wavelets(wav):
        v = np.asarray(d.fn(w.copy()))
        assert not np.isnan(v).any()
        assert np.array_equal(v[:5], np.zeros(5)) and v[-1] != 0


@pytest.mark.parametrize('case', [('gmw', dict(gamma=3, beta=60)), ('morlet', dict(mu=6))], ids=_id)
def test_float32_pair(case):
    """Same dtype as the wavelet; the values are those of the float64 pair to float32 accuracy (the
    argument rounded to float32 moves the value by up to ``max|psih''| * 12 eps32`` as well)."""
    name, opts = case
    w32, w64 = [Wavelet((name, dict(opts, dtype=dt))) for dt in ('float32', 'float64')]
    for d32, d64 in zip(derived_wavelets(w32), derived_wavelets(w64)):
        assert d32.dtype == 'float32' and d32.family is None
        a = np.asarray(d32.fn(W_AXIS.astype('float32')))
        b = np.asarray(d64.fn(W_AXIS.astype('float32').astype('float64')))
        assert a.dtype == np.float32
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()


def test_pair_is_made_once_per_configuration():
    """Plans are cached by the wavelet's key, which for a function is the function object: equal
    configurations must get the same pair."""
    a = derived_wavelets(Wavelet(('gmw', dict(gamma=3, beta=60))))
    b = derived_wavelets(Wavelet(('gmw', dict(gamma=3, beta=60))))
    c = derived_wavelets(Wavelet(('gmw', dict(gamma=3, beta=20))))
    assert a[0] is b[0] and a[1] is b[1]
    assert a[0].key() == b[0].key() and a[0].key() != c[0].key() and a[0].key() != a[1].key()


@pytest.mark.parametrize('wavelet', ['bump', 'cmhat', 'hhhat', ('gmw', {'order': 1}), ('gmw', {'order': 2}),
                                     lambda w: np.exp(-(w - 5)**2)],
                         ids=['bump', 'cmhat', 'hhhat', 'gmw-order1', 'gmw-order2', 'function'])
def test_unsupported_raise(wavelet):
    with pytest.raises(NotImplementedError, match="'gmw' with order=0.*'morlet'"):
        derived_wavelets(Wavelet(wavelet))
    with pytest.raises(TypeError):
        derived_wavelets('gmw')
