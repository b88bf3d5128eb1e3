# -*- coding: utf-8 -*-
"""Second-order synchrosqueezed CWT on the MI355X (Oberlin, Meignen 2017). No counterpart in the
reference.

`ssq_cwt` reassigns with ``Im(dWx / Wx) / 2pi``, an estimate that is exact for a pure tone and
biased on anything whose frequency moves inside the wavelet's time support. `ssq_cwt2` corrects
it with a per-point chirp-rate estimate built from two more transforms of the same signal, over
the banks ``psih'(w)`` and ``w psih(w)``; a linear chirp is then reassigned to its instantaneous
frequency. DESIGN.md section 4.5.4 states the map.
"""
import numpy as np

from . import algos
from .configs import EPS32, EPS64
from ._cwt import get_cwt_plan, _process_gmw_wavelet, _TDT
from ._ssq_cwt import _ssq_design
from .padding import PADTYPES
from .scales import _process_fs_and_t
from .ssqueezing import GRID_LIN, _check_ssqueezing_args
from .wavelets import Wavelet, derived_wavelets

__all__ = ['ssq_cwt2']


def _cwt_phase_map(x, wavelet, scales, nv, fs, t, ssq_freqs, padtype, maprange, gamma, chirp_tol,
                   cache_wavelet, get_w, order=2):
    """The host steps of `ssq_cwt2` up to its reassignment, for it and for `msst_cwt`: the
    checks, the design, the default of `gamma`, the plans, the executions and the map.
    ``order=2``: three executions and `phase_cwt2_gpu` (a wavelet with closed-form companions);
    ``order=1``: one and `phase_cwt_gpu` (any wavelet). Returns ``(Wx, w, ssq_freqs, scales_dt, const,
    grid, wavelet, fs)`` with `ssq_freqs` ascending, as the bins are taken."""
    if order not in (1, 2):
        raise ValueError("`order` must be 1 or 2 (got %r)" % (order,))
    if not hasattr(x, 'ndim'):
        raise TypeError("`x` must be a numpy array or torch Tensor "
                        "(got %s)" % type(x))
    elif x.ndim not in (1, 2):
        raise ValueError("`x` must be 1D or 2D (got x.ndim == %s)" % x.ndim)
    _check_ssqueezing_args('sum', maprange, wavelet, 'trig', None, get_w, transform='cwt')
    if padtype is not None and padtype not in PADTYPES:
        raise ValueError("`padtype` must be one of: %s (got %s)"
                         % (', '.join(PADTYPES), padtype))
    if nv is None and not isinstance(scales, np.ndarray):
        nv = 32
    N = x.shape[-1]
    dt, fs, t = _process_fs_and_t(fs, t, N)

    wavelet = _process_gmw_wavelet(wavelet, True)
    wavelet = Wavelet._init_if_not_isinstance(wavelet, N=N)
    # (raises for a wavelet without a closed form)
    companions = derived_wavelets(wavelet) if order == 2 else ()
    dtype = wavelet.dtype
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)

    scales_dt, ssq_freqs, const, grid, _ = _ssq_design(wavelet, scales, nv, N, dt, ssq_freqs,
                                                       maprange, bool(padtype is not None))
    use_cache = True if cache_wavelet is None else bool(cache_wavelet)
    xd = algos.to_device(x, _TDT[dtype]).detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    plans = [get_cwt_plan(wv, scales_dt, N, padtype, dt, True, B, cache=use_cache)
             for wv in (wavelet,) + companions]

    out = plans[0].execute(xd, want_dWx=True)
    Wx, dW = out['Wx'], out['dWx']
    if order == 1:
        return Wx, algos.phase_cwt_gpu(Wx, dW, gamma), ssq_freqs, scales_dt, const, grid, wavelet, fs
    out = plans[1].execute(xd, want_dWx=True)
    Wd, dWd = out['Wx'], out['dWx']
    dW3 = plans[2].execute(xd, want_dWx=True)['dWx']
    w = algos.phase_cwt2_gpu(Wx, dW, Wd, dWd, dW3, scales_dt, fs, gamma, chirp_tol)
    del dW, Wd, dWd, dW3, out
    return Wx, w, ssq_freqs, scales_dt, const, grid, wavelet, fs


def ssq_cwt2(x, wavelet='gmw', scales='log-piecewise', nv=None, fs=None, t=None,
             ssq_freqs=None, padtype='reflect', maprange='peak', gamma=None,
             chirp_tol=1e-3, astensor=True, flipud=True, cache_wavelet=None, get_w=False):
    """Second-order synchrosqueezed CWT. Arguments as `ssq_cwt`'s (``squeezing='sum'``,
    ``difftype='trig'``, ``order=0``), plus `chirp_tol`. Returns ``(Tx, Wx, ssq_freqs, scales[, w])``
    with `Tx`, `Wx` (and `w`) of shape ``(na, N)``; `x` is 1-D or ``(B, N)`` (a leading signal
    dimension on `Tx`, `Wx`, `w`; `get_w` is allowed for a batch). `Wx` is `ssq_cwt`'s.
    `wavelet`: ``'gmw'`` of order 0 or ``'morlet'`` (`wavelets.derived_wavelets`).

    With ``W, dW`` the CWT over ``psih(w)`` and its time derivative, ``Wd, dWd`` the same over
    ``psih'(w)``, ``dW3`` the time derivative of the CWT over ``w psih(w)`` and
    ``r = scales / fs``, per point::

        T   = -1j r Wd;  dT = -1j r dWd;  ddW = (1j / r) dW3
        den = W (W + dT) - T dW
        q   = (W ddW - dW^2) / den / (2pi j)                        # chirp rate, Hz/s
        w1  = Im(dW / W) / 2pi                                      # what ssq_cwt uses
        w2  = w1 - Im((W ddW - dW^2) T / (den W)) / 2pi
        w   = inf where |W| < gamma, else |w2| where |den| > chirp_tol |W|^2, else |w1|

    evaluated in float64 for both precisions and rounded once; ``den / W^2`` is 1 for a stationary
    tone and 0 for an impulse, where the chirp rate is undefined and the first-order estimate
    stands, as `phase_cwt` forms it. ``chirp_tol=np.inf`` gives `phase_cwt`'s `w` everywhere, bit
    for bit. `Tx` is ``indexed_sum_onfly(Wx, w, ssq_freqs, const, logscale, flipud)``: a cell's
    terms are added in ascending row order.

    Costs three plan executions (five planes are needed, six are made), the map and the
    reassignment. The outputs carry no `grad_fn`, whatever `x` requires."""
    Wx, w, ssq_freqs, scales_dt, const, grid, _, _ = _cwt_phase_map(
        x, wavelet, scales, nv, fs, t, ssq_freqs, padtype, maprange, gamma, chirp_tol,
        cache_wavelet, get_w)
    Tx = algos.indexed_sum_onfly(Wx, w, ssq_freqs, const, grid != GRID_LIN, flipud)

    # `scales` go high -> low, so frequencies are returned high -> low
    ssq_freqs = ssq_freqs[::-1]
    scales_out = scales_dt.squeeze()
    if not astensor:
        Tx, Wx, w = [a.cpu().numpy() for a in (Tx, Wx, w)]
    if get_w:
        return Tx, Wx, ssq_freqs, scales_out, w
    return Tx, Wx, ssq_freqs, scales_out
