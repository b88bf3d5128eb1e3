# -*- coding: utf-8 -*-
"""Multisynchrosqueezed STFT on the MI355X (MSST; Yu, Wang, Zhao, "Multisynchrosqueezing Transform",
IEEE Trans. Ind. Electron. 2019). No counterpart in the reference.

`ssq_stft` reassigns every coefficient to ``w(t, f)``, an estimate that is off by `chirp rate x group
delay` on a frequency-modulated component. `ssq_stft2` corrects it with four more transforms;
`msst_stft` needs none: seen through a Gaussian window, ``f -> w(t, f)`` is a contraction towards
the instantaneous frequency, so applying the map to its own output brings every point closer by
the same factor per pass. DESIGN.md section 4.5.8 states the definition; `ssq_multi_squeeze`
(include/ssq_hip.h) computes it in one kernel.
"""
from . import algos
from ._ssq_stft2 import _stft_phase_map

__all__ = ['msst_stft']


def msst_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, ssq_freqs=None,
              padtype='reflect', gamma=None, n_iter=10, interp='linear', order=1, chirp_tol=1e-3,
              dtype=None, astensor=True, flipud=False, get_w=False):
    """Multisynchrosqueezed STFT. Arguments as `ssq_stft2`'s, plus `n_iter`, `interp` and `order`.
    Returns ``(Tx, Sx, ssq_freqs, Sfs[, w_final])`` with `Tx`, `Sx` (and `w_final`) of shape
    ``(n_fft//2 + 1, n_hops)``; `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Tx`, `Sx`,
    `w_final`). `Sx` is `ssq_stft`'s.

    With `w` the phase transform -- `phase_stft`'s (``order=1``, one plan execution) or `ssq_stft2`'s
    (``order=2``, its three executions and `chirp_tol`) -- per column and point of row `k`::

        f = w[k]
        n_iter - 1 times:  f = w at the row position (f - Sfs[0]) / (Sfs[1] - Sfs[0])
        Tx[bin of f] += Sx[k] * const

    `w` between two rows is interpolated linearly (``interp='linear'``) or taken from the nearest
    row (``'nearest'``, the paper's form, which stalls once a pass moves a point by less than half
    a row). The iteration of a point stops at a fixed point, when `f` leaves the rows' range, or in
    front of a row below `gamma`. ``n_iter=1`` is `ssq_stft` with ``squeezing='sum'`` as
    `indexed_sum_onfly` computes it. `Tx` moves coefficients along the frequency axis of a column
    only, so `issq_stft` inverts it as it inverts `ssq_stft`'s. `w_final` holds the final frequency
    of every point, ``inf`` where ``|Sx| < gamma``.

    Costs `order`'s plan executions, the map and one kernel (`algos.multi_squeeze_gpu`). The outputs
    carry no `grad_fn`, whatever `x` requires."""
    Sx, w, ssq_freqs, Sfs, const = _stft_phase_map('msst_stft', x, window, n_fft, win_len, hop_len, fs, t,
                                                   ssq_freqs, padtype, gamma, chirp_tol, dtype, order)
    res = algos.multi_squeeze_gpu(Sx, w, Sfs, ssq_freqs, const, n_iter, interp, flipud, get_w=get_w)
    Tx, wf = res if get_w else (res, None)
    del w
    if flipud:
        ssq_freqs = ssq_freqs[::-1]
    if not astensor:
        Tx, Sx = Tx.cpu().numpy(), Sx.cpu().numpy()
        wf = wf.cpu().numpy() if get_w else None
    if get_w:
        return Tx, Sx, ssq_freqs, Sfs, wf
    return Tx, Sx, ssq_freqs, Sfs
