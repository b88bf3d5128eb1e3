# -*- coding: utf-8 -*-
"""The time-reassigned synchrosqueezed CWT on the MI355X: the CWT counterpart of `tssq_stft` (He, Cao, Zi, Zhou, Chen,
"Time-reassigned synchrosqueezing transform", 2019). No counterpart in the reference.

An impulse, a click or a dispersive wave packet is sharp in the high rows of a constant-Q analysis and smeared over a
wavelet's length in every row. `ssq_cwt` moves a coefficient along the frequency axis and cannot sharpen it;
``reassign_cwt(reassign='time')`` moves it along time but as an energy, without its phase. `tssq_cwt` moves the complex
coefficient of every point along its row to its group delay, after referring its phase to the signal's origin, so that
the terms that meet in a cell add coherently. DESIGN.md section 4.5.12 states the definition; `ssq_time_reassign_cwt`
(include/ssq_hip.h) computes it.
"""
from . import algos
from ._reassign_cwt import _derived_cwt_prelude, _t_hat
from .wavelets import row_frequencies, wavelet_time_std

__all__ = ['tssq_cwt']


def tssq_cwt(x, wavelet='gmw', scales='log-piecewise', nv=None, fs=None, t=None, padtype='reflect', gamma=None,
             max_shift=4., astensor=True, cache_wavelet=None, get_t=False):
    """Time-reassigned synchrosqueezed CWT. Arguments as `reassign_cwt`'s. Returns ``(Tx, Wx, freqs, scales[, t_hat])``
    with `Tx`, `Wx` (complex, and `t_hat`, real) of shape ``(na, N)``; `x` is 1-D or ``(B, N)`` (a leading signal
    dimension on `Tx`, `Wx` and `t_hat`). `Wx` is `ssq_cwt`'s; ``freqs = row_frequencies(wavelet, scales, fs)``, the
    rows' centre frequencies: a point stays in its row. `wavelet`: ``'gmw'`` of order 0 or ``'morlet'``
    (`wavelets.derived_wavelets`; others raise as they do there).

    With ``W`` the CWT over ``psih(w)`` and ``Wd`` the CWT over ``psih'(w)`` -- ``T = -1j r Wd``, ``r = scales / fs``,
    is the CWT taken with ``t psi(t)`` -- per point of row `i`, column `c` with ``|W| >= gamma``::

        d = rint(Im(Wd / W) scales[i])                          # columns to the group delay, Re(T / W) fs
        Tx[i, c + d] += W[i, c] exp(-2j pi freqs[i] / fs c)     # if |d| <= dmax[i] and the column exists

    ``dmax[i] = ceil(max_shift time_std scales[i])`` as in `reassign_cwt`. A CWT coefficient carries its phase relative
    to the wavelet's centre; the rotation refers it to the signal's origin, without which the terms of an impulse cancel.
    ``t_hat = times + Im(Wd / W) scales / fs``, the reassigned time of every point, is ``inf`` where ``|W| < gamma``.

    There is no inverse. A row's sum over time is the row sum of the rotated kept coefficients, ``sum_c W[i, c]
    exp(-2j pi freqs[i] c / fs)`` over the points that land: the signal's spectrum at ``freqs[i]`` seen through the
    wavelet -- what `tssq_stft`'s column sums are for an STFT row.

    The arithmetic is float64 for both precisions and a cell's sum is taken in signed fixed point
    (`algos.time_reassign_cwt_gpu`): it does not depend on the order of the additions, so the result is
    bit-reproducible. The outputs carry no `grad_fn`, whatever `x` requires."""
    wavelet, dt, fs, gamma, design, sc, execute = _derived_cwt_prelude(x, wavelet, scales, nv, fs, t, None, padtype, 'peak',
                                                                        gamma, cache_wavelet)
    Wx = execute(want_dWx=False)['Wx']
    Wd = execute(derived=True)['Wx']
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wavelet), max_shift)
    freqs = row_frequencies(wavelet, sc, fs)
    Tx = algos.time_reassign_cwt_gpu(Wx, Wd, sc, dmax, gamma, rot=algos.cwt_rotation_tables(freqs, Wx.shape[-1], fs))

    t_hat = _t_hat(Wx, Wd, sc, dt, gamma) if get_t else None
    del Wd

    scales_out = design[0].squeeze()
    if not astensor:
        Tx, Wx = Tx.cpu().numpy(), Wx.cpu().numpy()
        t_hat = t_hat.cpu().numpy() if t_hat is not None else None
    return (Tx, Wx, freqs, scales_out, t_hat) if get_t else (Tx, Wx, freqs, scales_out)
