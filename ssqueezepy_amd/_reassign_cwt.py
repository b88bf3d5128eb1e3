# -*- coding: utf-8 -*-
"""The reassigned scalogram on the MI355X (Auger, Flandrin, "Improving the readability of time-frequency and
time-scale representations by the reassignment method", IEEE Trans. SP 1995). No counterpart in the reference.

A constant-Q analysis has long wavelets at low frequencies and short ones at high frequencies, so one signal is
tone-like in some rows and impulse-like in others. `ssq_cwt` and `ssq_cwt2` move a coefficient along the frequency
axis: they sharpen the tone-like rows and leave the impulse-like rows smeared over the wavelet's length.
`reassign_cwt` moves the energy of every point along both axes at once, to the bin of its instantaneous frequency and
to its group delay. Like `reassign_stft` it gives up what the synchrosqueezed transforms keep: the result is an energy
distribution, real and non-negative, with no phase and no inverse. DESIGN.md section 4.5.10 states the definition;
`ssq_reassign_cwt` (include/ssq_hip.h) computes it.
"""
import numpy as np
import torch

from . import algos
from .configs import EPS32, EPS64
from ._cwt import get_cwt_plan, _process_gmw_wavelet, _TDT
from ._ssq_cwt import _ssq_design
from .padding import PADTYPES
from .scales import _process_fs_and_t
from .ssqueezing import _check_ssqueezing_args
from .wavelets import Wavelet, center_frequency, derived_wavelets, wavelet_time_std

__all__ = ['reassign_cwt']


def _derived_cwt_prelude(x, wavelet, scales, nv, fs, t, ssq_freqs, padtype, maprange, gamma, cache_wavelet):
    """What `reassign_cwt` and `tssq_cwt` do ahead of their kernel: the checks of `x` and `padtype`, the defaults of
    `nv`, `fs` / `t` and `gamma`, the wavelet with its ``psih'(w)`` companion and the design. Returns ``(wavelet, dt, fs,
    gamma, design, sc, execute)``: `design` is `_ssq_design`'s, `sc` the scales as float64, and ``execute(derived=False,
    **kw)`` runs the plan of the wavelet -- of the companion with `derived` -- on `x` and hands back its planes."""
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
    if gamma is None:
        gamma = 10 * (EPS64 if wavelet.dtype == 'float64' else EPS32)

    design = _ssq_design(wavelet, scales, nv, N, dt, ssq_freqs, maprange, bool(padtype is not None))
    use_cache = True if cache_wavelet is None else bool(cache_wavelet)
    xd = algos.to_device(x, _TDT[wavelet.dtype]).detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    sc = np.asarray(design[0], dtype=np.float64).reshape(-1)

    def execute(derived=False, **kw):
        return get_cwt_plan(companion if derived else wavelet, design[0], N, padtype, dt, True, B,
                            cache=use_cache).execute(xd, **kw)
    return wavelet, dt, fs, gamma, design, sc, execute


def _t_hat(Wx, Wd, sc, dt, gamma):
    """``times + Re(T / W)``, the reassigned time of every point, ``inf`` where ``|Wx| < gamma``: ``T = -1j r Wd``, ``r =
    sc dt``, so ``Re(T / W) = r Im(Wd / W)``."""
    dtype = np.float32 if Wx.dtype == torch.complex64 else np.float64
    times = torch.as_tensor((np.arange(Wx.shape[-1]) * dt).astype(dtype), device=Wx.device)
    r = torch.as_tensor((sc * dt).astype(dtype), device=Wx.device)[:, None]
    t_hat = times + (Wd / Wx).imag * r
    return torch.where(torch.abs(Wx) < gamma, torch.full_like(t_hat, float('inf')), t_hat)


def reassign_cwt(x, wavelet='gmw', scales='log-piecewise', nv=None, fs=None, t=None, ssq_freqs=None,
                 padtype='reflect', maprange='peak', gamma=None, reassign='both', max_shift=4.,
                 astensor=True, flipud=True, cache_wavelet=None, get_maps=False):
    """Reassigned scalogram. Arguments as `ssq_cwt2`'s, plus `reassign` and `max_shift`. Returns
    ``(Rx, Wx, ssq_freqs, scales[, f_hat, t_hat])`` with `Rx` (real), `Wx` (and `f_hat`, `t_hat`) of shape ``(na, N)``;
    `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Rx`, `Wx` and the maps). `Wx` is `ssq_cwt`'s. `wavelet`:
    ``'gmw'`` of order 0 or ``'morlet'`` (`wavelets.derived_wavelets`).

    With ``W, dW`` the CWT over ``psih(w)`` and its time derivative, ``Wd`` the CWT over ``psih'(w)`` and ``T = -1j r
    Wd``, ``r = scales / fs`` -- the CWT taken with ``t psi(t)`` -- per point of row `i`, column `c` with ``|W| >=
    gamma``::

        k = the bin of |Im(dW / W)| / 2pi on `ssq_freqs`       # as `ssq_cwt` takes it; mirrored by `flipud`
        d = rint(Re(T / W) fs)                                  # columns to the group delay
        Rx[k, c + d] += |W[i, c]|^2 const[i]                    # if |d| <= dmax[i] and the column exists

    ``const`` is `ssq_cwt`'s row weight (``da / a``), so a bin's sum approximates ``int |W|^2 da / a`` on
    ``'log-piecewise'`` scales too; ``dmax[i] = ceil(max_shift time_std scales[i])``, `time_std` the standard deviation
    of ``|psi(t)|^2`` at scale 1 (`wavelets.wavelet_time_std`): a centre of gravity further out is no estimate.
    ``reassign='freq'`` keeps ``d = 0`` (one plan execution instead of two), ``'time'`` keeps ``k = i``.
    ``f_hat = |Im(dW / W)| / 2pi`` and ``t_hat = times + Re(T / W)``, the reassigned frequency and time of every
    point, are ``inf`` where ``|W| < gamma`` (and `None` for an axis that is off).

    The arithmetic is float64 for both precisions and a cell's sum is taken in fixed point
    (`algos.reassign_cwt_gpu`): it does not depend on the order of the additions, so the result is bit-reproducible,
    and it lies below the exact sum by less than (the cell's terms) x ``2^-sh`` before the one rounding to the
    output's precision. The outputs carry no `grad_fn`, whatever `x` requires."""
    if reassign not in ('both', 'freq', 'time'):
        raise ValueError("`reassign` must be 'both', 'freq' or 'time' (got %r)" % (reassign,))
    _check_ssqueezing_args('sum', maprange, wavelet, 'trig', None, False, transform='cwt')
    wavelet, dt, fs, gamma, design, sc, execute = _derived_cwt_prelude(x, wavelet, scales, nv, fs, t, ssq_freqs, padtype,
                                                                        maprange, gamma, cache_wavelet)
    scales_dt, ssq_freqs, const = design[:3]
    freq, time = reassign != 'time', reassign != 'freq'

    out = execute(want_dWx=freq)
    Wx, dW = out['Wx'], out.get('dWx')
    Wd = dmax = None
    if time:
        Wd = execute(derived=True)['Wx']
        dmax = algos.reassign_cwt_dmax(sc, wavelet_time_std(wavelet), max_shift)
    # (the LDS windows go where the rows' own centre frequencies lie on the grid: `maprange` and a caller's `ssq_freqs`
    # may put them anywhere)
    home = algos.reassign_cwt_home(sc, ssq_freqs, flipud, freq, wc=center_frequency(wavelet, kind='peak-ct'), fs=fs)
    Rx = algos.reassign_cwt_gpu(Wx, dW, Wd, sc, const, dmax, ssq_freqs, gamma, flipud=flipud, home=home)

    f_hat = t_hat = None
    if get_maps:
        if freq:
            f_hat = torch.abs((dW / Wx).imag) / (2 * np.pi)
            f_hat = torch.where(torch.abs(Wx) < gamma, torch.full_like(f_hat, float('inf')), f_hat)
        if time:
            t_hat = _t_hat(Wx, Wd, sc, dt, gamma)
    del dW, Wd, out

    # `scales` go high -> low, so frequencies are returned high -> low
    ssq_freqs = ssq_freqs[::-1]
    scales_out = scales_dt.squeeze()
    if not astensor:
        Rx, Wx = Rx.cpu().numpy(), Wx.cpu().numpy()
        f_hat = f_hat.cpu().numpy() if f_hat is not None else None
        t_hat = t_hat.cpu().numpy() if t_hat is not None else None
    return (Rx, Wx, ssq_freqs, scales_out, f_hat, t_hat) if get_maps else (Rx, Wx, ssq_freqs, scales_out)
