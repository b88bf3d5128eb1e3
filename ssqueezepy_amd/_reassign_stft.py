# -*- coding: utf-8 -*-
"""The reassigned spectrogram on the MI355X (Kodera, Gendrin, de Villedary, "Analysis of time-varying signals
with small BT values", IEEE Trans. ASSP 1978; Auger, Flandrin, "Improving the readability of time-frequency and
time-scale representations by the reassignment method", IEEE Trans. SP 1995). No counterpart in the reference.

`ssq_stft` and its relatives move a coefficient along the frequency axis, `tssq_stft` along the time axis. A
component that is neither a tone nor an impulse -- a frequency-modulated tone, a fast chirp -- is smeared along
both, and either one-axis transform leaves part of the smear. `reassign_stft` moves the energy of every point
along both axes at once, to its instantaneous frequency and its group delay. It gives up what the
synchrosqueezed transforms keep: the result is an energy distribution, real and non-negative, with no phase and
no inverse. DESIGN.md section 4.5.9 states the definition; `ssq_reassign2d` (include/ssq_hip.h) computes it.
"""
import numpy as np
import torch

from . import algos
from .configs import EPS32, EPS64
from ._stft import _stft_setup
from ._ssq_stft import _make_Sfs
from ._tssq_stft import _tau_plan

__all__ = ['reassign_stft']


def reassign_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, padtype='reflect',
                  gamma=None, reassign='both', dtype=None, astensor=True, get_maps=False):
    """Reassigned spectrogram. Arguments as `ssq_stft`'s (``modulated=True``). Returns
    ``(Rx, Sx, Sfs, times[, f_hat, t_hat])`` with `Rx` (real), `Sx` (and `f_hat`, `t_hat`) of shape
    ``(n_fft//2 + 1, n_hops)``; `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Rx`, `Sx` and the maps).
    `Sx` is `stft`'s, `Sfs` the rows' frequencies and ``times[c] = c hop_len / fs`` the columns' times.

    With ``V^h`` the STFT taken with window `h`, `g` the analysis window, `g'` its derivative and ``tau`` the
    window's time axis in seconds (0 at the centre), per point of row `k`, column `c` with ``|V^g| >= gamma``::

        m = rint(-Im(V^{g'} / V^g) / (2 pi) / (fs / n_fft))     # rows to the instantaneous frequency
        d = rint(Re(V^{tau g} / V^g) fs / hop_len)              # columns to the group delay
        Rx[|k + m|, c + d] += |V^g[k, c]|^2                     # if |d| <= half a window and the cell exists

    ``reassign='freq'`` keeps ``d = 0`` (one plan execution instead of two), ``'time'`` keeps ``m = 0``.
    ``f_hat = Sfs - Im(V^{g'} / V^g) / (2 pi)`` and ``t_hat = times + Re(V^{tau g} / V^g)``, the reassigned
    frequency and time of every point, are ``inf`` where ``|V^g| < gamma`` (and `None` for an axis that is off).

    The arithmetic is float64 for both precisions. A cell's sum is taken in fixed point
    (`algos.reassign2d_gpu`): it does not depend on the order of the additions, so the result is bit-reproducible,
    and it lies below the exact sum by less than (the cell's terms) x ``2^-sh``, ``sh = 62 - bit_length(rows
    min(2 dmax + 1, n_hops)) - frexp(max |V^g|^2)[1]`` -- for a plane of 129 x 4096 at hop 1 and a cell of a hundred
    terms less than 2.8e-12 of the plane's largest energy -- before the one rounding to `dtype`.

    Costs two plan executions (one for ``'freq'``) and three launches. The outputs carry no `grad_fn`, whatever
    `x` requires."""
    if reassign not in ('both', 'freq', 'time'):
        raise ValueError("`reassign` must be 'both', 'freq' or 'time' (got %r)" % (reassign,))
    plan, xd, fs, dtype = _stft_setup(x, window, n_fft, win_len, hop_len, fs, t, padtype, True, dtype)
    xd = xd.detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    freq, time = reassign != 'time', reassign != 'freq'
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)

    out = plan.execute(xd, want_dSx=freq)
    Sx, dSx = out['Sx'], out.get('dSx')
    Vtg = None
    if time:
        # (the first plan was made by _stft_setup, which has already issued the NOLA warnings for `g`)
        Vtg = _tau_plan(plan, window, win_len, hop_len, fs, padtype, dtype, B).execute(xd)['Sx']
    Rx = algos.reassign2d_gpu(Sx, dSx, Vtg, plan.n_fft, hop_len, fs, gamma)

    Sfs = _make_Sfs(plan.rows, fs, dtype)
    times = (np.arange(plan.n_hops) * hop_len / fs).astype(dtype)
    f_hat = t_hat = None
    if get_maps:
        low = torch.abs(Sx) < gamma
        if freq:
            f_hat = torch.as_tensor(Sfs, device=Sx.device)[:, None] - (dSx / Sx).imag / (2 * np.pi)
            f_hat = torch.where(low, torch.full_like(f_hat, float('inf')), f_hat)
        if time:
            t_hat = torch.as_tensor(times, device=Sx.device) + (Vtg / Sx).real
            t_hat = torch.where(low, torch.full_like(t_hat, float('inf')), t_hat)
    del dSx, Vtg
    if not astensor:
        Rx, Sx = Rx.cpu().numpy(), Sx.cpu().numpy()
        f_hat = f_hat.cpu().numpy() if f_hat is not None else None
        t_hat = t_hat.cpu().numpy() if t_hat is not None else None
    return (Rx, Sx, Sfs, times, f_hat, t_hat) if get_maps else (Rx, Sx, Sfs, times)
