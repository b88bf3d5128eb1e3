# -*- coding: utf-8 -*-
"""ConceFT -- "concentration of frequency and time" (Daubechies, Wang, Wu 2016): multitaper
synchrosqueezing of the STFT on the MI355X. No counterpart in the reference.

Synchrosqueezing sharpens a clean signal; on a noisy one the reassignment scatters the noise into
spurious ridges. ConceFT takes `J` orthonormal windows, forms `Q` random unit combinations of the
`J` STFTs (by linearity each is the STFT with the combined window: no further transforms),
synchrosqueezes every combination and averages the magnitudes: the signal's ridges add up, the
noise's artefacts -- which depend on the window -- do not. DESIGN.md section 4.5.5 states the
definition; `ssq_conceft` (include/ssq_hip.h) computes it in one kernel.
"""
import numpy as np

from . import algos
from .configs import EPS32, EPS64, defaults
from ._stft import _centered, get_window, get_stft_plan, _TDT
from ._ssq_stft import _make_Sfs
from .padding import PADTYPES
from .scales import infer_scaletype, _process_fs_and_t

__all__ = ['conceft_stft', 'hermite_windows', 'draw_projections']


def _hermite_functions(n, t):
    """The orthonormal Hermite functions ``h_0 .. h_{n-1}`` at `t`, float64, by the three-term recurrence."""
    h = np.empty((n, len(t)))
    h[0] = np.pi ** -.25 * np.exp(-.5 * t * t)
    if n > 1:
        h[1] = np.sqrt(2.) * t * h[0]
    for k in range(2, n):
        h[k] = np.sqrt(2. / k) * t * h[k - 1] - np.sqrt((k - 1.) / k) * h[k - 2]
    return h


def hermite_windows(n_tapers, win_len, n_fft=None, t_max=6., dtype=None):
    """``(H, dH)``, each ``(n_tapers, n_fft)``: the first `n_tapers` Hermite functions sampled at
    ``t[m] = (m - win_len//2) dt``, ``dt = 2 t_max / win_len``, scaled by ``sqrt(dt)`` so that the
    rows of `H` are orthonormal (``H @ H.T = I`` up to the tails cut off at ``+- t_max``), and their
    derivatives per sample in closed form, ``h_k' = sqrt(k/2) h_{k-1} - sqrt((k+1)/2) h_{k+1}``
    times `dt`. Both are zero-padded to `n_fft` (default `win_len`) on the side `get_window` pads.
    Computed in float64, cast to `dtype` (default float64) at the end. ``1 <= n_tapers <= 8``."""
    J = int(n_tapers)
    if not 1 <= J <= 8:
        raise ValueError("`n_tapers` must be 1 .. 8 (got %s)" % (n_tapers,))
    win_len = int(win_len)
    n_fft = win_len if n_fft is None else int(n_fft)
    if win_len > n_fft:
        raise ValueError("Can't have `win_len > n_fft` ({} > {})".format(win_len, n_fft))
    dt = 2. * float(t_max) / win_len
    t = (np.arange(win_len) - win_len // 2) * dt
    h = _hermite_functions(J + 1, t)
    dh = np.empty((J, win_len))
    for k in range(J):
        dh[k] = -np.sqrt((k + 1) / 2.) * h[k + 1]
        if k:
            dh[k] += np.sqrt(k / 2.) * h[k - 1]
    H = np.stack([_centered(w, win_len, n_fft) for w in h[:J] * np.sqrt(dt)])
    dH = np.stack([_centered(w, win_len, n_fft) for w in dh * (dt * np.sqrt(dt))])
    dtype = 'float64' if dtype is None else dtype
    return H.astype(dtype), dH.astype(dtype)


def draw_projections(n_proj, n_tapers, seed=0):
    """The raw draw behind ``conceft_stft(proj=None)``: ``g = default_rng(seed).standard_normal((n_proj,
    n_tapers, 2))``, ``g[..., 0] + 1j g[..., 1]`` -- (Q, J) complex128, not yet normalised."""
    g = np.random.default_rng(seed).standard_normal((int(n_proj), int(n_tapers), 2))
    return g[..., 0] + 1j * g[..., 1]


def _unit_rows(proj, J):
    proj = np.asarray(proj, dtype=np.complex128)
    if proj.ndim != 2 or proj.shape[1] != J or not proj.shape[0]:
        raise ValueError("`proj` must be (Q, %d), Q >= 1 (got %s)" % (J, proj.shape))
    norm = np.sqrt((proj.real ** 2 + proj.imag ** 2).sum(axis=1, keepdims=True))
    if not (np.isfinite(norm).all() and (norm > 0).all()):
        raise ValueError("every row of `proj` must be finite and non-zero")
    return proj / norm


def conceft_stft(x, n_tapers=3, n_proj=30, windows=None, proj=None, seed=0, n_fft=None, win_len=None,
                 hop_len=1, fs=None, t=None, ssq_freqs=None, padtype='reflect', gamma=None, t_max=6.,
                 average='abs', dtype=None, astensor=True, flipud=False):
    """Multitaper synchrosqueezed STFT (ConceFT). Returns ``(Cx, Sxs, ssq_freqs, Sfs)``: `Cx`
    ``(n_fft//2 + 1, n_hops)`` -- real for ``average='abs'``, complex for ``'complex'`` --, `Sxs` the
    list of the `J` STFTs; `x` is 1-D or ``(B, N)`` (a leading signal dimension on `Cx` and `Sxs`).

    `windows`: None -> `hermite_windows(n_tapers, win_len, n_fft, t_max)`, or a ``(J, win_len)`` array
    of windows of the caller's (their derivatives are taken as `get_window` takes them). `proj`: None
    -> `draw_projections(n_proj, J, seed)`, the same bits for the same seed, or a ``(Q, J)`` complex
    array; either way every row is normalised to unit 2-norm in float64. With ``V_j`` the STFT taken
    with window `j` and ``dV_j`` the one taken with its derivative, per projection `q`::

        Vq  = sum_j proj[q, j] V_j,   dVq = sum_j proj[q, j] dV_j
        w   = |Sfs[k] - Im(dVq / Vq) / 2pi|        where |Vq| >= gamma
        Tq  = the reassignment of Vq by w onto `ssq_freqs` (a cell's terms in ascending row order)
        Cx  = mean_q |Tq|   ('abs')      or      mean_q Tq   ('complex')

    in float64 for both precisions, rounded once, in one kernel that reads the `2J` planes once
    and writes `Cx` (`algos.conceft_gpu`). `Tq` carries no weight: it is `ssq_stft2`'s `Tx` without
    its constant factor ``ssq_freqs[1] - ssq_freqs[0]``. `Sfs`, `gamma` and `ssq_freqs` (linear only)
    are as in `ssq_stft2`. Costs `J` plan executions and the kernel. The outputs carry no `grad_fn`."""
    if (isinstance(ssq_freqs, np.ndarray) and
            infer_scaletype(ssq_freqs)[0] != 'linear'):
        raise ValueError("`ssq_freqs` must be linearly distributed "
                         "for `conceft_stft`")
    if average not in ('abs', 'complex'):
        raise ValueError("`average` must be 'abs' or 'complex' (got %r)" % (average,))
    assert x.ndim in (1, 2)
    if padtype not in PADTYPES:
        raise ValueError("`padtype` must be one of: %s (got %s)" % (', '.join(PADTYPES), padtype))
    N = x.shape[-1]
    _, fs, _ = _process_fs_and_t(fs, t, N)
    n_fft = n_fft or min(N // hop_len, 512)
    if dtype is None:
        dtype = defaults('stft')['dtype']
    dtype = str(np.dtype(dtype))
    if windows is None:
        win_len = win_len or n_fft
        H, dH = hermite_windows(n_tapers, win_len, n_fft, t_max, dtype)
    else:
        windows = np.asarray(windows)
        if windows.ndim != 2 or not 1 <= windows.shape[0] <= 8:
            raise ValueError("`windows` must be (J, win_len), 1 <= J <= 8 (got %s)" % (windows.shape,))
        win_len = win_len or windows.shape[1]
        pairs = [get_window(np.asarray(w, dtype='float64'), win_len, n_fft, derivative=True, dtype=dtype)
                 for w in windows]
        H, dH = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    J = len(H)
    proj = _unit_rows(draw_projections(n_proj, J, seed) if proj is None else proj, J)

    xd = algos.to_device(x, _TDT[dtype]).detach()
    B = xd.shape[0] if xd.ndim == 2 else 1
    Sxs, dSxs = [], []
    for j in range(J):
        plan = get_stft_plan(N, n_fft, hop_len, H[j], dH[j], fs, padtype, True, dtype, B)
        out = plan.execute(xd, want_dSx=True)
        Sxs.append(out['Sx'])
        dSxs.append(out['dSx'])

    Sfs = _make_Sfs(plan.rows, fs, dtype)
    if gamma is None:
        gamma = 10 * (EPS64 if dtype == 'float64' else EPS32)
    if ssq_freqs is None:
        ssq_freqs = Sfs
    ssq_freqs = np.asarray(ssq_freqs)
    Cx = algos.conceft_gpu(Sxs, dSxs, Sfs, proj, ssq_freqs, gamma, flipud, average)
    if flipud:
        ssq_freqs = ssq_freqs[::-1]
    if not astensor:
        Cx = Cx.cpu().numpy()
        Sxs = [S.cpu().numpy() for S in Sxs]
    return Cx, Sxs, ssq_freqs, Sfs
