# -*- coding: utf-8 -*-
"""ConceFT for the CWT (Daubechies, Wang, Wu 2016, section 2): multitaper synchrosqueezing with
generalized Morse wavelets of increasing order as the orthogonal tapers. No counterpart in the
reference.

`conceft_stft` (`_conceft.py`) says what ConceFT is for. The paper states it first for the CWT:
`J` wavelets that are mutually orthogonal and of equal norm -- `wavelets.morse_wavelets`, the
orders ``0 .. J-1`` of one GMW --, `Q` random unit combinations of the `J` CWTs, each
synchrosqueezed as `ssq_cwt` synchrosqueezes, the magnitudes averaged. DESIGN.md section 4.5.6
states the definition; `ssq_conceft_cwt` (include/ssq_hip.h) computes it in one kernel.
"""
import numpy as np

from . import algos
from .configs import EPS32, EPS64
from ._cwt import get_cwt_plan, _process_gmw_wavelet, _TDT
from ._conceft import draw_projections, _unit_rows
from ._ssq_cwt import _ssq_design
from .padding import PADTYPES
from .scales import _process_fs_and_t
from .ssqueezing import _check_ssqueezing_args
from .wavelets import Wavelet, morse_wavelets

__all__ = ['conceft_cwt']


def conceft_cwt(x, wavelet='gmw', n_tapers=3, n_proj=30, proj=None, seed=0, scales='log-piecewise',
                nv=None, fs=None, t=None, ssq_freqs=None, padtype='reflect', maprange='peak',
                gamma=None, average='abs', astensor=True, flipud=True, cache_wavelet=None):
    """Multitaper synchrosqueezed CWT (ConceFT). Returns ``(Cx, Wxs, ssq_freqs, scales)``: `Cx`
    ``(na, N)`` -- real for ``average='abs'``, complex for ``'complex'`` --, `Wxs` the list of the
    `J` CWTs; `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Cx` and `Wxs`).

    `wavelet`: a GMW (name, ``(name, dict)`` or `Wavelet`, ``norm='bandpass'``); the tapers are its
    orders ``0 .. n_tapers-1`` (`wavelets.morse_wavelets`), ``1 <= n_tapers <= 8``. `proj`: None ->
    `draw_projections(n_proj, J, seed)`, the same bits for the same seed, or a ``(Q, J)`` complex
    array; either way every row is normalised to unit 2-norm in float64. `scales`, `nv`, `fs`, `t`,
    `ssq_freqs`, `padtype`, `maprange`, `gamma`, `flipud`, `cache_wavelet`: as in `ssq_cwt`; the
    scales, the frequency grid and the rows' weights `const` are designed with the order-0 wavelet
    and shared by all orders, as `cwt_higher_order` shares its scales. With ``W_j, dW_j`` the CWT
    over the order-`j` wavelet and its time derivative, per projection `q`::

        Wq  = sum_j proj[q, j] W_j,   dWq = sum_j proj[q, j] dW_j
        w   = |Im(dWq / Wq)| / 2pi                 where |Wq| >= gamma
        Tq  = the reassignment of Wq * const by w onto `ssq_freqs` (a cell's terms in ascending row order)
        Cx  = mean_q |Tq|   ('abs')      or      mean_q Tq   ('complex')

    in float64 for both precisions, rounded once, in one kernel that reads the `2J` planes once and
    writes `Cx` (`algos.conceft_cwt_gpu`). With ``n_tapers=1`` and ``average='complex'`` this is
    `ssq_cwt`'s `Tx` evaluated in float64. `ssq_freqs` is returned high to low, as `ssq_cwt2` returns
    it. Costs `J` plan executions and the kernel. The outputs carry no `grad_fn`."""
    if not hasattr(x, 'ndim'):
        raise TypeError("`x` must be a numpy array or torch Tensor (got %s)" % type(x))
    elif x.ndim not in (1, 2):
        raise ValueError("`x` must be 1D or 2D (got x.ndim == %s)" % x.ndim)
    if average not in ('abs', 'complex'):
        raise ValueError("`average` must be 'abs' or 'complex' (got %r)" % (average,))
    _check_ssqueezing_args('sum', maprange, wavelet, 'trig', None, False, transform='cwt')
    if padtype is not None and padtype not in PADTYPES:
        raise ValueError("`padtype` must be one of: %s (got %s)" % (', '.join(PADTYPES), padtype))
    if nv is None and not isinstance(scales, np.ndarray):
        nv = 32
    N = x.shape[-1]
    dt, fs, t = _process_fs_and_t(fs, t, N)

    wavelet = _process_gmw_wavelet(wavelet, True)
    tapers = morse_wavelets(Wavelet._init_if_not_isinstance(wavelet, N=N), n_tapers)
    J = len(tapers)
    dtype = tapers[0].dtype
    proj = _unit_rows(draw_projections(n_proj, J, seed) if proj is None else proj, J)
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)

    scales_dt, ssq_freqs, const, _, _ = _ssq_design(tapers[0], scales, nv, N, dt, ssq_freqs, maprange,
                                                    bool(padtype is not None))
    use_cache = True if cache_wavelet is None else bool(cache_wavelet)
    xd = algos.to_device(x, _TDT[dtype]).detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    Wxs, dWxs = [], []
    for wv in tapers:
        out = get_cwt_plan(wv, scales_dt, N, padtype, dt, True, B, cache=use_cache).execute(xd, want_dWx=True)
        Wxs.append(out['Wx'])
        dWxs.append(out['dWx'])
    Cx = algos.conceft_cwt_gpu(Wxs, dWxs, proj, ssq_freqs, const, gamma, flipud, average)

    # `scales` go high -> low, so frequencies are returned high -> low
    ssq_freqs = ssq_freqs[::-1]
    if not astensor:
        Cx = Cx.cpu().numpy()
        Wxs = [W.cpu().numpy() for W in Wxs]
    return Cx, Wxs, ssq_freqs, scales_dt.squeeze()
