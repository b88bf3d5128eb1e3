# -*- coding: utf-8 -*-
"""Time-reassigned synchrosqueezed STFT on the MI355X (TSST; He, Cao, Zi, Zhou, Chen, "Time-reassigned
synchrosqueezing transform: the algorithm and its applications in mechanical signal processing",
MSSP 2019). No counterpart in the reference.

`ssq_stft` and its relatives move a coefficient along the frequency axis, which suits tones and slow
chirps. An impulse, a click or a dispersive wave packet lies along the time axis of the plane, and
frequency reassignment leaves it smeared over a window length. `tssq_stft` is the counterpart: every
coefficient moves along the time axis, within its row, to its local group delay. DESIGN.md section
4.5.7 states the definition; `ssq_time_reassign` (include/ssq_hip.h) computes it in one kernel.
"""
import numpy as np
import torch

from . import algos
from .configs import EPS32, EPS64
from ._stft import _stft_setup, _window_design, get_stft_plan
from ._ssq_stft import _make_Sfs
from ._ssq_stft2 import _second_order_windows

__all__ = ['tssq_stft']


def _tau_plan(plan, window, win_len, hop_len, fs, padtype, dtype, B):
    """The plan that transforms with ``tau g`` (no derivative window), `g` being the window `plan` was made with."""
    if win_len is None:
        win_len = len(window) if isinstance(window, np.ndarray) else plan.n_fft
    g, dg, _ = _window_design(window, win_len, plan.n_fft, hop_len, dtype)
    (tg, _), _ = _second_order_windows(g, dg, plan.n_fft, fs)
    return get_stft_plan(plan.N, plan.n_fft, hop_len, tg, None, fs, padtype, True, dtype, B)


def tssq_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, padtype='reflect',
              gamma=None, dtype=None, astensor=True, get_t=False):
    """Time-reassigned synchrosqueezed STFT. Arguments as `ssq_stft`'s (``modulated=True``). Returns
    ``(Tx, Sx, Sfs, times[, t_hat])`` with `Tx`, `Sx` (and `t_hat`) of shape ``(n_fft//2 + 1, n_hops)``;
    `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Tx`, `Sx`, `t_hat`). `Sx` is `stft`'s,
    `Sfs` the rows' frequencies and ``times[c] = c hop_len / fs`` the columns' times.

    With ``V^h`` the STFT taken with window `h`, `g` the analysis window and ``tau`` the window's
    time axis in seconds (0 at the centre), per point of row `k`, column `c`::

        s   = Re(V^{tau g} / V^g)                  # the local group delay relative to the frame centre, s
        d   = rint(s fs / hop_len)                 # columns; kept where |V^g| >= gamma and |d| <= half a window
        Tx[k, c + d] += Sx[k, c] e^{-2 pi i k c hop_len / n_fft}

    in float64 for both precisions, a cell's terms in ascending `c`, rounded once
    (`algos.time_reassign_gpu`). ``t_hat = times + s``, the reassigned time of every point, is
    ``inf`` where ``|V^g| < gamma``.

    `Sx` carries the phase relative to its frame's centre; the rotation refers every term to the
    signal's origin, so `Tx[k, :]` carries the absolute phase, ``Sx[k, c] e^{-2 pi i k c hop / n_fft}``:
    the terms of an impulse that meet in a cell add coherently instead of cancelling, and a row's sum
    over time equals the row sum of the rotated kept coefficients. That marginal is the signal's
    spectrum seen through the window; inverting it fully needs ``n_fft >= N``, so no inverse is offered.

    Costs two plan executions and the kernel. The outputs carry no `grad_fn`, whatever `x` requires."""
    plan, xd, fs, dtype = _stft_setup(x, window, n_fft, win_len, hop_len, fs, t, padtype, True, dtype)
    xd = xd.detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    # the first plan was made by _stft_setup, which has already issued the NOLA warnings -- for `g`,
    # the only window they are about
    plan_t = _tau_plan(plan, window, win_len, hop_len, fs, padtype, dtype, B)
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)

    Sx = plan.execute(xd)['Sx']
    Vtg = plan_t.execute(xd)['Sx']
    Tx = algos.time_reassign_gpu(Sx, Vtg, plan.n_fft, hop_len, fs, gamma)

    Sfs = _make_Sfs(plan.rows, fs, dtype)
    times = (np.arange(plan.n_hops) * hop_len / fs).astype(dtype)
    t_hat = None
    if get_t:
        s = (Vtg / Sx).real
        t_hat = torch.as_tensor(times, device=s.device) + s
        t_hat = torch.where(torch.abs(Sx) < gamma, torch.full_like(t_hat, float('inf')), t_hat)
    del Vtg
    if not astensor:
        Tx, Sx = Tx.cpu().numpy(), Sx.cpu().numpy()
        t_hat = t_hat.cpu().numpy() if get_t else None
    return (Tx, Sx, Sfs, times, t_hat) if get_t else (Tx, Sx, Sfs, times)
