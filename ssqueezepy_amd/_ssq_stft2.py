# -*- coding: utf-8 -*-
"""Second-order synchrosqueezed STFT on the MI355X (Oberlin, Meignen, Perrier 2015; Behera,
Meignen, Oberlin 2018). No counterpart in the reference.

`ssq_stft` reassigns with ``Sfs - Im(dSx / Sx) / 2pi``, an estimate that is off by `chirp rate x
group delay` on anything but a pure tone. `ssq_stft2` corrects it with a per-point chirp-rate
estimate built from four more transforms of the same signal; a linear chirp is then reassigned
to its instantaneous frequency exactly. DESIGN.md section 4.5.3 states the map.
"""
import numpy as np

from . import algos
from .configs import EPS32, EPS64
from ._stft import _stft_setup, _spectral_derivative, _window_design, get_stft_plan
from ._ssq_stft import _make_Sfs
from .scales import infer_scaletype

__all__ = ['ssq_stft2']


def _second_order_windows(g, dg, n_fft, fs):
    """The window pairs of the second and third plan, as `StftPlan` takes them (it multiplies the
    second of a pair by `fs`): ``(tau g, tau g')`` and ``(g, g'' fs)``. `g`, `dg`: the pair of the
    first plan (`get_window(derivative=True)`), so `g''` is the derivative of the very `g'` that
    plan transforms with. ``tau[m] = (m - n_fft//2) / fs``."""
    tau = (np.arange(n_fft) - n_fft // 2) / fs
    g64, dg64 = np.asarray(g, dtype='float64'), np.asarray(dg, dtype='float64')
    return (tau * g64, tau * dg64), (g64, _spectral_derivative(dg64) * fs)


def _stft_phase_map(name, x, window, n_fft, win_len, hop_len, fs, t, ssq_freqs, padtype, gamma,
                    chirp_tol, dtype, order=2):
    """The host steps of `ssq_stft2` up to its reassignment, for it and for `msst_stft` (`name` in the
    message): the check of `ssq_freqs`, the plans, the defaults of `gamma`, `ssq_freqs` and `const`,
    the executions and the map. ``order=2``: three executions and `phase_stft2_gpu`; ``order=1``: one
    and `phase_stft_gpu`. Returns ``(Sx, w, ssq_freqs, Sfs, const)``."""
    if order not in (1, 2):
        raise ValueError("`order` must be 1 or 2 (got %r)" % (order,))
    if (isinstance(ssq_freqs, np.ndarray) and
            infer_scaletype(ssq_freqs)[0] != 'linear'):
        raise ValueError("`ssq_freqs` must be linearly distributed "
                         "for `%s`" % name)
    plan, xd, fs, dtype = _stft_setup(x, window, n_fft, win_len, hop_len, fs, t,
                                      padtype, True, dtype)
    xd = xd.detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    # the pair the first plan was made with: a cache hit after _stft_setup, which has already
    # issued the NOLA warnings -- for `g`, the only window they are about
    n_fft = plan.n_fft
    if win_len is None:
        win_len = len(window) if isinstance(window, np.ndarray) else n_fft
    plans = []
    if order == 2:
        g, dg, _ = _window_design(window, win_len, n_fft, hop_len, dtype)
        pair_t, pair_dd = _second_order_windows(g, dg, n_fft, fs)
        plans = [get_stft_plan(plan.N, n_fft, hop_len, wa, wb, fs, padtype, True, dtype, B)
                 for wa, wb in (pair_t, pair_dd)]

    Sfs = _make_Sfs(plan.rows, fs, dtype)
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)
    if ssq_freqs is None:
        ssq_freqs = Sfs
    ssq_freqs = np.asarray(ssq_freqs)
    const = (ssq_freqs[1] - ssq_freqs[0])

    out = plan.execute(xd, want_dSx=True)
    Sx, Vdg = out['Sx'], out['dSx']
    if order == 1:
        return Sx, algos.phase_stft_gpu(Sx, Vdg, Sfs, gamma), ssq_freqs, Sfs, const
    out = plans[0].execute(xd, want_dSx=True)
    Vtg, Vtdg = out['Sx'], out['dSx']
    Vddg = plans[1].execute(xd, want_dSx=True)['dSx']
    w = algos.phase_stft2_gpu(Sx, Vdg, Vddg, Vtg, Vtdg, Sfs, gamma, chirp_tol)
    del Vdg, Vddg, Vtg, Vtdg, out
    return Sx, w, ssq_freqs, Sfs, const


def ssq_stft2(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None,
              ssq_freqs=None, padtype='reflect', gamma=None, chirp_tol=1e-3,
              dtype=None, astensor=True, flipud=False, get_w=False):
    """Second-order synchrosqueezed STFT. Arguments as `ssq_stft`'s (``modulated=True``,
    ``squeezing='sum'``), plus `chirp_tol`. Returns ``(Tx, Sx, ssq_freqs, Sfs[, w])`` with `Tx`,
    `Sx` (and `w`) of shape ``(n_fft//2 + 1, n_hops)``; `x` is 1-D or ``(B, N)`` (a leading signal
    dimension on `Tx`, `Sx`, `w`; `get_w` is allowed for a batch). `Sx` is `ssq_stft`'s.

    With ``V^h`` the STFT taken with window `h`, `g` the analysis window, ``g'`` its derivative
    and ``tau`` the window's time axis in seconds (0 at the centre), per point::

        w1  = Sfs[k] - Im(V^{g'} / V^g) / 2pi                       # what ssq_stft uses
        den = V^{tau g} V^{g'} - V^{tau g'} V^g
        q   = (V^{g''} V^g - (V^{g'})^2) / den / (2pi j)            # chirp rate, Hz/s
        w2  = Re(w1c - q V^{tau g} / V^g),  w1c = Sfs[k] + 1j V^{g'} / V^g / 2pi
        w   = inf where |V^g| < gamma, else |w2| where |den| > chirp_tol |V^g|^2, else |w1|

    evaluated in float64 for both precisions and rounded once; ``den / (V^g)^2`` is the
    derivative of the local group delay -- 1 for a stationary tone, 0 for an impulse, where the
    chirp rate is undefined and the first-order estimate stands, as `phase_stft` forms it (float32:
    its float32 numerator). ``chirp_tol=np.inf`` gives `phase_stft`'s `w` everywhere, bit for bit. `Tx` is ``indexed_sum_onfly(Sx, w, ssq_freqs, const, False,
    flipud)``: a cell's terms are added in ascending row order, whatever `SSQ_TILE_ORDER` says.

    Costs three plan executions (five transforms are needed, six are made), the map and the
    reassignment. The outputs carry no `grad_fn`, whatever `x` requires."""
    Sx, w, ssq_freqs, Sfs, const = _stft_phase_map('ssq_stft2', x, window, n_fft, win_len, hop_len, fs, t,
                                                   ssq_freqs, padtype, gamma, chirp_tol, dtype)
    Tx = algos.indexed_sum_onfly(Sx, w, ssq_freqs, const, False, flipud)
    if flipud:
        ssq_freqs = ssq_freqs[::-1]
    if not astensor:
        Tx, Sx, w = [a.cpu().numpy() for a in (Tx, Sx, w)]
    if get_w:
        return Tx, Sx, ssq_freqs, Sfs, w
    return Tx, Sx, ssq_freqs, Sfs
