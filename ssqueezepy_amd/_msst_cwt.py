# -*- coding: utf-8 -*-
"""Multisynchrosqueezed CWT on the MI355X (MSST; Yu, Wang, Zhao, "Multisynchrosqueezing Transform",
IEEE Trans. Ind. Electron. 2019, carried over to the wavelet transform). No counterpart in the
reference.

`ssq_cwt` reassigns every coefficient to ``w(t, a)``, an estimate that is off on a
frequency-modulated component by `chirp rate x group delay` of the row's wavelet. `ssq_cwt2`
corrects it with two more plan executions and takes only wavelets with closed-form companions;
`msst_cwt` needs neither: a Morlet row at scale `a` is a Gaussian-window STFT of width ``a sigma``
read at ``wc / a``, so ``f -> w(t, f)`` is a contraction towards the instantaneous frequency in
every row, with a factor that depends on the row, and applying the map to its own output brings
every point closer pass by pass. Where the frequency moves faster than a row's wavelet can follow
(a modulation period of about 100 samples at the default design) the map is no contraction in the
affected rows and more passes buy nothing: that is the method's limit. DESIGN.md section 4.5.11
states the definition; `ssq_multi_squeeze_cwt` (include/ssq_hip.h) computes it in one kernel.
"""
from . import algos
from ._ssq_cwt2 import _cwt_phase_map
from .wavelets import row_frequencies

__all__ = ['msst_cwt']


def msst_cwt(x, wavelet='gmw', scales='log-piecewise', nv=None, fs=None, t=None, ssq_freqs=None,
             padtype='reflect', maprange='peak', gamma=None, n_iter=10, interp='linear', order=1,
             chirp_tol=1e-3, astensor=True, flipud=True, cache_wavelet=None, get_w=False):
    """Multisynchrosqueezed CWT. Arguments as `ssq_cwt2`'s, plus `n_iter`, `interp` and `order`.
    Returns ``(Tx, Wx, ssq_freqs, scales[, w_final])`` with `Tx`, `Wx` (and `w_final`) of shape
    ``(na, N)``; `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Tx`, `Wx`, `w_final`).
    `Wx` is `ssq_cwt`'s.

    With `w` the phase transform -- `phase_cwt`'s (``order=1``, one plan execution, any wavelet) or
    `ssq_cwt2`'s (``order=2``, its three executions, its wavelets and `chirp_tol`) -- and ``fr[i] =
    wc fs / (2 pi scales[i])`` the rows' centre frequencies (`wavelets.row_frequencies`), per column
    and point of row `i`::

        f = w[i]
        n_iter - 1 times:  f = w at the place of f between the two rows of fr around it
        Tx[bin of f] += Wx[i] * const[i]

    `w` between two rows is interpolated linearly in frequency (``interp='linear'``) or taken from
    the nearer row (``'nearest'``, the paper's form, which stalls once a pass moves a point by less
    than half a row). The iteration of a point stops at a fixed point, when `f` leaves the rows'
    range, or in front of a row below `gamma`. ``n_iter=1`` is `ssq_cwt` with ``squeezing='sum'``
    as `indexed_sum_onfly` computes it. `Tx` moves coefficients along the frequency axis of a
    column only, so `issq_cwt` inverts it as it inverts `ssq_cwt`'s. `w_final` holds the final
    frequency of every point, ``inf`` where ``|Wx| < gamma``.

    Costs `order`'s plan executions (1 or 3), the map and one kernel
    (`algos.multi_squeeze_cwt_gpu`). The outputs carry no `grad_fn`, whatever `x` requires."""
    Wx, w, ssq_freqs, scales_dt, const, _, wavelet, fs = _cwt_phase_map(
        x, wavelet, scales, nv, fs, t, ssq_freqs, padtype, maprange, gamma, chirp_tol, cache_wavelet,
        False, order)
    fr = row_frequencies(wavelet, scales_dt, fs)
    res = algos.multi_squeeze_cwt_gpu(Wx, w, fr, ssq_freqs, const, n_iter, interp, flipud, get_w=get_w)
    Tx, wf = res if get_w else (res, None)
    del w

    # `scales` go high -> low, so frequencies are returned high -> low
    ssq_freqs = ssq_freqs[::-1]
    scales_out = scales_dt.squeeze()
    if not astensor:
        Tx, Wx = Tx.cpu().numpy(), Wx.cpu().numpy()
        wf = wf.cpu().numpy() if get_w else None
    if get_w:
        return Tx, Wx, ssq_freqs, scales_out, wf
    return Tx, Wx, ssq_freqs, scales_out
