# -*- coding: utf-8 -*-
"""`hermite_windows`: the orthonormal Hermite tapers of `conceft_stft` and their derivatives (host NumPy)."""
import numpy as np
import pytest
from conftest import report_measured
from ssqueezepy_amd._conceft import hermite_windows, _hermite_functions
from ssqueezepy_amd._stft import get_window

J, WIN, T_MAX = 4, 256, 6.


def test_rows_are_orthonormal():
    """``H H^T = I`` to 1e-8: the sum over the grid is the trapezoid rule on a function that decays like
    ``exp(-t^2)``, exact to rounding but for the tails beyond ``t_max``, about ``h_3(6)^2`` ~ 1e-11."""
    H, _ = hermite_windows(J, WIN, t_max=T_MAX)
    assert H.shape == (J, WIN) and H.dtype == np.float64
    err = float(np.abs(H @ H.T - np.eye(J)).max())
    report_measured('conceft_hermite_gram', max_err=err)
    assert err <= 1e-8


def test_derivative_matches_a_centred_difference_on_a_finer_grid():
    """`dH` against ``(h(t + e) - h(t - e)) / 2e * dt`` of the same closed form, ``e = dt / 8``. The centred
    difference is off by ``e^2 / 6 max|h'''|``; with ``h_k'' = (t^2 - 2k - 1) h_k`` the third derivative is
    ``2 t h_k + (t^2 - 2k - 1) h_k'``, bounded on the grid through the closed forms themselves. The bound asserted
    is that truncation term (in the window's scaling) plus the rounding of the difference quotient,
    ``4 eps max|h| / e``."""
    _, dH = hermite_windows(J, WIN, t_max=T_MAX)
    dt = 2 * T_MAX / WIN
    e = dt / 8
    t = (np.arange(WIN) - WIN // 2) * dt
    hp, hm, h = _hermite_functions(J + 1, t + e), _hermite_functions(J + 1, t - e), _hermite_functions(J + 1, t)
    worst = 0.
    for k in range(J):
        fd = (hp[k] - hm[k]) / (2 * e) * dt * np.sqrt(dt)
        d1 = -np.sqrt((k + 1) / 2.) * h[k + 1] + (np.sqrt(k / 2.) * h[k - 1] if k else 0.)
        d3 = np.abs(2 * t * h[k] + (t * t - 2 * k - 1) * d1).max()
        # (h''' varies over [t - e, t + e]: a factor 2 covers it on this grid, where e = 0.006)
        bound = (2 * e * e / 6 * d3 + 4 * np.finfo(float).eps * np.abs(h[k]).max() / e) * dt * np.sqrt(dt)
        err = float(np.abs(fd - dH[k]).max())
        report_measured('conceft_hermite_derivative', k=k, max_err=err, bound=float(bound))
        assert err <= bound, (k, err, bound)
        worst = max(worst, err / bound)
    assert worst > 1e-3            # the bound is of the error's order, not a blanket


def test_parity_about_the_centre():
    H, dH = hermite_windows(J, WIN, t_max=T_MAX)
    c = WIN // 2
    for k in range(J):
        s = (-1) ** k
        assert np.allclose(H[k, c + 1:], s * H[k, c - 1:0:-1], rtol=0, atol=1e-15)
        assert np.allclose(dH[k, c + 1:], -s * dH[k, c - 1:0:-1], rtol=0, atol=1e-15)


@pytest.mark.parametrize('win_len, n_fft', [(100, 128), (101, 128), (100, 127)])
def test_padding_side_is_get_windows(win_len, n_fft):
    H, dH = hermite_windows(3, win_len, n_fft)
    H0, dH0 = hermite_windows(3, win_len)
    for k in range(3):
        assert np.array_equal(H[k], get_window(H0[k], win_len, n_fft))
        assert np.array_equal(dH[k], get_window(dH0[k], win_len, n_fft))
    assert hermite_windows(2, 64, dtype='float32')[0].dtype == np.float32
    for bad in (0, 9):
        with pytest.raises(ValueError):
            hermite_windows(bad, 64)
