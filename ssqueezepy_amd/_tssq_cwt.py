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
import numpy as np
import torch

from . import algos
from .configs import EPS32, EPS64
from ._cwt import get_cwt_plan, _process_gmw_wavelet, _TDT
from ._ssq_cwt import _ssq_design
from .padding import PADTYPES
from .scales import _process_fs_and_t
from .wavelets import Wavelet, derived_wavelets, row_frequencies, wavelet_time_std

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
    if not hasattr(x, 'ndim'):
        raise TypeError("`x` must be a numpy array or torch Tensor "
                        "(got %s)" % type(x))
    elif x.ndim not in (1, 2):
        raise ValueError("`x` must be 1D or 2D (got x.ndim == %s)" % x.ndim)
    if padtype is not None and padtype not in PADTYPES:
        raise ValueError("`padtype` must be one of: %s (got %s)"
                         % (', '.join(PADTYPES), padtype))
    if nv is None and not isinstance(scales, np.ndarray):
        nv = 32
    N = x.shape[-1]
    dt, fs, t = _process_fs_and_t(fs, t, N)

    wavelet = _process_gmw_wavelet(wavelet, True)
    wavelet = Wavelet._init_if_not_isinstance(wavelet, N=N)
    companion = derived_wavelets(wavelet)[0]    # raises for a wavelet without a closed form
    dtype = wavelet.dtype
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)

    scales_dt = _ssq_design(wavelet, scales, nv, N, dt, None, 'peak', bool(padtype is not None))[0]
    use_cache = True if cache_wavelet is None else bool(cache_wavelet)
    xd = algos.to_device(x, _TDT[dtype]).detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    sc = np.asarray(scales_dt, dtype=np.float64).reshape(-1)

    Wx = get_cwt_plan(wavelet, scales_dt, N, padtype, dt, True, B, cache=use_cache).execute(xd, want_dWx=False)['Wx']
    Wd = get_cwt_plan(companion, scales_dt, N, padtype, dt, True, B, cache=use_cache).execute(xd)['Wx']
    dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wavelet), max_shift)
    freqs = row_frequencies(wavelet, sc, fs)
    Tx = algos.time_reassign_cwt_gpu(Wx, Wd, sc, dmax, gamma, rot=algos.cwt_rotation_tables(freqs, N, fs))

    t_hat = None
    if get_t:
        low = torch.abs(Wx) < gamma
        times = torch.as_tensor((np.arange(N) * dt).astype(dtype), device=Wx.device)
        r = torch.as_tensor((sc * dt).astype(dtype), device=Wx.device)[:, None]
        t_hat = times + (Wd / Wx).imag * r                      # Re(-1j r Wd / W) = r Im(Wd / W)
        t_hat = torch.where(low, torch.full_like(t_hat, float('inf')), t_hat)
    del Wd

    scales_out = scales_dt.squeeze()
    if not astensor:
        Tx, Wx = Tx.cpu().numpy(), Wx.cpu().numpy()
        t_hat = t_hat.cpu().numpy() if t_hat is not None else None
    return (Tx, Wx, freqs, scales_out, t_hat) if get_t else (Tx, Wx, freqs, scales_out)
