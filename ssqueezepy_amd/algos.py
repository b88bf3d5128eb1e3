# -*- coding: utf-8 -*-
"""Kernel-level seam: the reference's `algos.py` entry points, on the MI355X.

Same names, argument meaning and error behaviour as the functions the reference's
transforms call (ssqueezepy/algos.py): `ssqueeze_fast` (126-150),
`indexed_sum_onfly` (153-169), `indexed_sum_bins` (the same sum from a caller's bin map: no counterpart in the reference), `phase_cwt_gpu` (743-781), `phase_stft_gpu`
(818-856), `phase_stft2_gpu` and `phase_cwt2_gpu` (the second-order maps: no counterpart in the reference), `conceft_gpu` and `conceft_cwt_gpu` (multitaper synchrosqueezing, likewise), `time_reassign_gpu` (time-reassigned synchrosqueezing, likewise), `multi_squeeze_gpu` and `multi_squeeze_cwt_gpu` (multisynchrosqueezing, likewise), `reassign2d_gpu` (the reassigned spectrogram, likewise), `reassign_cwt_gpu` (the reassigned scalogram, likewise), `time_reassign_cwt_gpu` (the time-reassigned synchrosqueezed CWT, likewise), `replace_under_abs` (498-579) and `buffer` (utils/stft_utils.py:20-66).
Inputs may be NumPy arrays (uploaded) or torch tensors; outputs are torch tensors
on the GPU. Every function is a thin marshalling layer over one C-ABI call of
libssq_hip.so, launched on torch's current stream -- there is no CPU
implementation behind them.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, params5, F32, F64

__all__ = ['ssqueeze_fast', 'ssqueeze_adjoint', 'indexed_sum_onfly', 'indexed_sum_bins', 'reassign_route', 'phase_cwt_gpu', 'phase_stft_gpu', 'phase_stft2_gpu', 'phase_cwt2_gpu', 'conceft_gpu', 'conceft_cwt_gpu', 'time_reassign_gpu', 'multi_squeeze_gpu', 'multi_squeeze_cwt_gpu', 'reassign2d_gpu', 'reassign_cwt_gpu', 'time_reassign_cwt_gpu', 'cwt_rotation_tables', 'time_reassign_cwt_shift',
           'replace_under_abs', 'buffer', 'pad_signal_gpu', 'to_device', 'colsum_real', 'colsum_adjoint',
           'band_colsum', 'band_colsum_adjoint', 'istft_gpu', 'istft_adjoint_gpu', 'istft_algo']

_CDT = {torch.complex64: F32, torch.complex128: F64,
        torch.float32: F32, torch.float64: F64}


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("ssqueezepy_amd needs a ROCm GPU (torch.cuda.is_available()"
                           " is False); there is no CPU fallback.")


def device():
    _require_gpu()
    return torch.device('cuda', torch.cuda.current_device())


def stream():
    return torch.cuda.current_stream().cuda_stream


def to_device(x, dtype=None):
    """NumPy array / torch tensor -> contiguous torch tensor on the current GPU whose storage
    holds the values `x` denotes: a lazy conjugate / negative (`x.conj()`, `x.conj().imag`) is
    materialised -- `.contiguous()` alone keeps the bit, and `data_ptr()` then addresses the
    unconjugated values. Differentiable; a plain contiguous device tensor is returned as it is."""
    dev = device()
    if isinstance(x, np.ndarray):
        if not x.flags.c_contiguous:
            x = np.ascontiguousarray(x)
        x = torch.from_numpy(x)
    elif not isinstance(x, torch.Tensor):
        raise TypeError("expected numpy array or torch Tensor (got %s)" % type(x))
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x.to(dev).resolve_conj().resolve_neg().contiguous()


def _check_out(out, like, dtype=None, message="`out` must be a contiguous GPU tensor of `Wx`'s shape and dtype"):
    """An `out=` argument is written through its raw pointer as a dense array of `like`'s shape, of `like`'s dtype
    or of `dtype`."""
    if not (isinstance(out, torch.Tensor) and out.shape == like.shape and out.dtype == (dtype or like.dtype)
            and out.is_cuda and out.is_contiguous() and not out.is_conj()):
        raise ValueError(message)


def ones_like(x):
    return torch.ones_like(x)


def cabs(x):
    return torch.abs(x).to(x.dtype)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _real_of(cdtype):
    return torch.float32 if cdtype == torch.complex64 else torch.float64


def _shape3(t):
    if t.ndim == 2:
        return 1, t.shape[0], t.shape[1]
    if t.ndim == 3:
        return t.shape
    raise ValueError("expected a 2D or 3D array (got ndim=%d)" % t.ndim)


def _complex_planes(name, first, **optional):
    """``(first, [optional planes], (B, rows, n))``: `first` on the device, complex, and the `optional` planes in its
    dtype and of its shape; None passes through (`name` and the keywords in the messages)."""
    first = to_device(first)
    if first.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`%s` must be complex64 or complex128 (got %s)" % (name, first.dtype))
    shape = _shape3(first)
    planes = []
    for key, P in optional.items():
        if P is not None:
            P = to_device(P, first.dtype)
            if P.shape != first.shape:
                raise ValueError("`%s` and `%s` must share one shape (got %s and %s)"
                                 % (name, key, tuple(first.shape), tuple(P.shape)))
        planes.append(P)
    return first, planes, shape


def _row_vector(name, v, rows, dtype=None, scalar_ok=False):
    """`v` as a contiguous host vector with one entry per row, of `dtype` (None: its own); with `scalar_ok` one value
    stands for every row (`name` in the message)."""
    v = v.detach().cpu().numpy() if hasattr(v, 'detach') else v
    v = np.asarray(v).reshape(-1)
    if not (v.size == rows or (scalar_ok and v.size == 1)):
        raise ValueError("`%s` must have one entry per row (%d != %d)" % (name, v.size, rows))
    return np.array(np.broadcast_to(v, (rows,)), dtype=dtype)      # (a copy: contiguous and writable)


def _row_dmax(dmax, rows):
    """The rows' largest displacements as the fixed-point entries take them: int32, host."""
    dm = _row_vector('dmax', dmax, rows, np.int64)
    if (dm < np.iinfo(np.int32).min).any() or (dm > np.iinfo(np.int32).max).any():
        raise ValueError("`dmax` must fit 32 bits")
    return dm.astype(np.int32)


def _fixed_point_buffers(like, B, words=1):
    """``(acc, peak)`` of a fixed-point scatter: the int64 sums, `words` per point of `like`, and a word per signal."""
    shape = tuple(like.shape) + ((words,) if words > 1 else ())
    return (torch.empty(shape, dtype=torch.int64, device=like.device),
            torch.empty((B,), dtype=torch.int64, device=like.device))


def _const_vector(const, na, cdtype):
    """Per-row weights as the reference materialises them (algos.py:66-79):
    scalar -> vector in the data dtype; a float64 vector weighting complex64 data
    stays float64 (the accumulate is then done in double, like NumPy/numba do)."""
    rdt = _real_of(cdtype)
    if isinstance(const, torch.Tensor):
        const = const.detach().cpu().numpy()
    const = np.asarray(const)
    if const.size != na:
        vec = torch.full((na,), float(const), dtype=rdt)
        return vec.to(device()), 0
    const = const.reshape(-1)
    if cdtype == torch.complex64 and const.dtype == np.float64:
        return torch.from_numpy(np.ascontiguousarray(const)).to(device()), 1
    return torch.from_numpy(np.ascontiguousarray(const)).to(rdt).to(device()), 0


def _grid(ssq_freqs, logscale):
    from .ssqueezing import ssq_grid_params
    kind, p = ssq_grid_params(ssq_freqs, logscale)
    return kind, params5(p)


def ssqueeze_fast(Wx, dWx, ssq_freqs, const, logscale=False, flipud=False,
                  gamma=None, out=None, Sfs=None, parallel=None, get_k=False):
    """Fused phase transform + nearest-bin search + accumulate: for every point
    with ``|Wx| > gamma``, ``Tx[k, j] += Wx[i, j] * const[i]``.
    Reference: `ssqueeze_fast`, ssqueezepy/algos.py:126-150."""
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    lib = _lib.load()
    Wx, dWx = to_device(Wx), to_device(dWx)
    if Wx.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`Wx` must be complex64 or complex128 (got %s)" % Wx.dtype)
    dWx = dWx.to(Wx.dtype)
    if Wx.shape != dWx.shape:
        raise ValueError("`Wx` and `dWx` shapes differ: %s vs %s"
                         % (tuple(Wx.shape), tuple(dWx.shape)))
    B, na, n = _shape3(Wx)
    if out is None:
        out = torch.empty_like(Wx)
    else:
        _check_out(out, Wx)
    cst, c64 = _const_vector(const, na, Wx.dtype)
    kind, p = _grid(ssq_freqs, logscale)
    sfs = None
    if Sfs is not None:
        sfs = to_device(Sfs, _real_of(Wx.dtype))
    kmap = (torch.empty((B, na, n), dtype=torch.int32, device=Wx.device)
            if get_k else None)
    check(lib.ssq_ssqueeze(_CDT[Wx.dtype], _ptr(Wx), _ptr(dWx), _ptr(sfs),
                           _ptr(out), _ptr(cst), c64, B, na, n, float(gamma), kind,
                           p, int(bool(flipud)), _ptr(kmap), stream()))
    if get_k:
        return out, kmap.reshape(Wx.shape)
    return out


def ssqueeze_adjoint(Wx, dWx, gTx, ssq_freqs, const, logscale=False, flipud=False,
                     gamma=None, Sfs=None, out=None, accumulate=False):
    """Adjoint of `ssqueeze_fast` with the bins held fixed: ``gWx[i, j] = const[i] *
    gTx[k(i, j), j]`` where ``|Wx[i, j]| > gamma`` and 0 elsewhere, `k` the bin `ssqueeze_fast`
    puts the point in (same arguments). The bins are integers, piecewise constant in the data,
    so this is the exact gradient of `Tx` w.r.t. `Wx` wherever it exists. `out` with
    `accumulate=True` is added to (a gradient that reaches `Wx` directly is already there);
    otherwise it is overwritten / allocated."""
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    lib = _lib.load()
    Wx, dWx = to_device(Wx), to_device(dWx)
    if Wx.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`Wx` must be complex64 or complex128 (got %s)" % Wx.dtype)
    dWx = dWx.to(Wx.dtype)
    gTx = to_device(gTx, Wx.dtype).resolve_conj().contiguous()
    if Wx.shape != dWx.shape or Wx.shape != gTx.shape:
        raise ValueError("`Wx`, `dWx` and `gTx` shapes differ: %s, %s, %s"
                         % (tuple(Wx.shape), tuple(dWx.shape), tuple(gTx.shape)))
    B, na, n = _shape3(Wx)
    if out is None:
        if accumulate:
            raise ValueError("`accumulate=True` needs `out`")
        out = torch.empty_like(Wx)
    else:
        _check_out(out, Wx)
    cst, c64 = _const_vector(const, na, Wx.dtype)
    kind, p = _grid(ssq_freqs, logscale)
    sfs = None
    if Sfs is not None:
        sfs = to_device(Sfs, _real_of(Wx.dtype))
    check(lib.ssq_ssqueeze_adjoint(_CDT[Wx.dtype], _ptr(Wx), _ptr(dWx), _ptr(sfs), _ptr(gTx),
                                   _ptr(out), int(bool(accumulate)), _ptr(cst), c64, B, na, n,
                                   float(gamma), kind, p, int(bool(flipud)), stream()))
    return out


def indexed_sum_onfly(Wx, w, ssq_freqs, const=1, logscale=False, flipud=False,
                      out=None, parallel=None):
    """Nearest-bin search + accumulate from a precomputed phase transform `w`
    (``inf`` = skip). Reference: `indexed_sum_onfly`, ssqueezepy/algos.py:153-169."""
    lib = _lib.load()
    Wx = to_device(Wx)
    w = to_device(w, _real_of(Wx.dtype))
    if Wx.shape != w.shape:
        raise ValueError("`Wx` and `w` shapes differ")
    B, na, n = _shape3(Wx)
    if out is None:
        out = torch.empty_like(Wx)
    else:
        _check_out(out, Wx)
    cst, c64 = _const_vector(const, na, Wx.dtype)
    kind, p = _grid(ssq_freqs, logscale)
    check(lib.ssq_indexed_sum(_CDT[Wx.dtype], _ptr(Wx), _ptr(w), _ptr(out),
                              _ptr(cst), c64, B, na, n, kind, p,
                              int(bool(flipud)), stream()))
    return out


SKIP_BIN = 0xFFFF               # `indexed_sum_bins`: the map's "no bin" entry


def indexed_sum_bins(Wx, k, const=1, out=None):
    """Accumulate into bins the caller supplies: ``Tx[k[i, j], j] += Wx[i, j] * const[i]`` (`ssq_indexed_sum_bins`,
    include/ssq_hip.h). `Wx`: (na, n) or (B, na, n) complex; `k`: a uint16 array or tensor of `Wx`'s shape, the bin of
    every point after any flip, ``SKIP_BIN`` (0xFFFF) = skip; `const` as `indexed_sum_onfly`'s. This is the bin source
    of every float64 `ssq_cwt`: by default a cell is the float64 sum of its terms in arrival order, rounded once, where
    `reassign_route` says 'f64'; ``SSQ_TILE_ORDER=ordered`` gives `indexed_sum_onfly`'s ordered sums. The kernels trust
    the map, so a map with an entry that is neither ``SKIP_BIN`` nor ``< na`` is refused here, before any launch."""
    lib = _lib.load()
    Wx = to_device(Wx)
    if Wx.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`Wx` must be complex64 or complex128 (got %s)" % Wx.dtype)
    if isinstance(k, np.ndarray):
        if k.dtype != np.uint16:
            raise TypeError("`k` must be uint16 (got %s)" % k.dtype)
        k = torch.from_numpy(np.ascontiguousarray(k))
    elif not isinstance(k, torch.Tensor):
        raise TypeError("expected numpy array or torch Tensor (got %s)" % type(k))
    if k.dtype != torch.uint16:
        raise TypeError("`k` must be uint16 (got %s)" % k.dtype)
    if Wx.shape != k.shape:
        raise ValueError("`Wx` and `k` shapes differ: %s vs %s" % (tuple(Wx.shape), tuple(k.shape)))
    B, na, n = _shape3(Wx)
    if na >= SKIP_BIN:
        raise ValueError("a bin map addresses fewer than %d rows (got %d)" % (SKIP_BIN, na))
    if out is not None:
        _check_out(out, Wx)
    k = k.to(device()).contiguous()
    # one reduction on the device: the largest entry that is not the skip mark (int16's bit pattern: torch reduces no
    # uint16; a mark becomes -1, entries of 0x8000 and more become negative and are caught below)
    ks = k.view(torch.int16)
    bad = ((ks != -1) & ((ks < 0) | (ks >= na))).any()
    if bool(bad):
        raise ValueError("`k` holds a bin that is neither 0x%X (skip) nor < %d" % (SKIP_BIN, na))
    if out is None:
        out = torch.empty_like(Wx)
    cst, c64 = _const_vector(const, na, Wx.dtype)
    check(lib.ssq_indexed_sum_bins(_CDT[Wx.dtype], _ptr(Wx), _ptr(k), _ptr(out), _ptr(cst), c64, B, na, n, stream()))
    return out


def reassign_route(dtype, binsrc, na, n, ordered=None, kmap=False):
    """What `ssqueeze_fast` (``binsrc='dwx'``), `indexed_sum_onfly` (``'w'``) and `indexed_sum_bins` / the plans' bin
    maps (``'bins'``) launch for a shape: ``(kernel, cols, wavefronts)`` with `kernel` one of 'tile16', 'tile', 'f64',
    'global' (`ssq_reassign_route`, include/ssq_hip.h; no device call). `ordered`: None -> what ``SSQ_TILE_ORDER`` says
    now; `kmap`: the caller asks for the bin map (`get_k`)."""
    import os
    code = F32 if str(dtype) in ('float32', 'torch.float32', 'torch.complex64', 'complex64') else F64
    src = {'dwx': _lib.BIN_FROM_DWX, 'w': _lib.BIN_FROM_W, 'bins': _lib.BIN_FROM_KIDX}[binsrc]
    if ordered is None:
        ordered = os.environ.get('SSQ_TILE_ORDER') == 'ordered'
    kern, cols, waves = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_lib.load().ssq_reassign_route(code, src, int(na), int(n), int(bool(ordered)), int(bool(kmap)),
                                         ctypes.byref(kern), ctypes.byref(cols), ctypes.byref(waves)))
    return _lib.REASSIGN_KERNELS[kern.value], cols.value, waves.value


def phase_cwt_gpu(Wx, dWx, gamma):
    """``w = inf where |Wx| < gamma else |Im(dWx / Wx)| / 2pi``.
    Reference: `phase_cwt_gpu`, ssqueezepy/algos.py:743-781."""
    lib = _lib.load()
    Wx, dWx = to_device(Wx), to_device(dWx)
    dWx = dWx.to(Wx.dtype)
    B, na, n = _shape3(Wx)
    w = torch.empty(Wx.shape, dtype=_real_of(Wx.dtype), device=Wx.device)
    check(lib.ssq_phase_cwt(_CDT[Wx.dtype], _ptr(Wx), _ptr(dWx), _ptr(w), B, na, n,
                            float(gamma), stream()))
    return w


def phase_stft_gpu(Sx, dSx, Sfs, gamma):
    """``w = inf where |Sx| < gamma else |Sfs[i] - Im(dSx / Sx) / 2pi|``.
    Reference: `phase_stft_gpu`, ssqueezepy/algos.py:818-856."""
    lib = _lib.load()
    Sx, dSx = to_device(Sx), to_device(dSx)
    dSx = dSx.to(Sx.dtype)
    sfs = to_device(Sfs, _real_of(Sx.dtype))
    B, na, n = _shape3(Sx)
    w = torch.empty(Sx.shape, dtype=_real_of(Sx.dtype), device=Sx.device)
    check(lib.ssq_phase_stft(_CDT[Sx.dtype], _ptr(Sx), _ptr(dSx), _ptr(sfs), _ptr(w),
                             B, na, n, float(gamma), stream()))
    return w


def _five_planes(name, first, *rest):
    """The five planes of a second-order map on the device in the complex dtype of `first` (`name` in the message),
    their ``(B, rows, n)`` and the output plane `w`, allocated."""
    first = to_device(first)
    if first.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`%s` must be complex64 or complex128 (got %s)" % (name, first.dtype))
    planes = [first] + [to_device(V, first.dtype) for V in rest]
    for V in planes[1:]:
        if V.shape != first.shape:
            raise ValueError("the five transforms must share one shape (got %s and %s)"
                             % (tuple(first.shape), tuple(V.shape)))
    return planes, _shape3(first), torch.empty(first.shape, dtype=_real_of(first.dtype), device=first.device)


def phase_stft2_gpu(Vg, Vdg, Vddg, Vtg, Vtdg, Sfs, gamma, chirp_tol=1e-3):
    """Second-order phase transform of the STFT (`ssq_stft2_phase`, include/ssq_hip.h) from the
    transforms taken with the windows ``g, g' fs, g'' fs^2, tau g, tau g' fs``, each (rows, n) or (B, rows, n)::

        w1  = Sfs[i] - Im(Vdg / Vg) / 2pi
        den = Vtg Vdg - Vtdg Vg
        w2  = w1 - Im((Vddg Vg - Vdg^2) Vtg / (den Vg)) / 2pi
        w   = inf where |Vg| < gamma else |w2| where |den| > chirp_tol |Vg|^2 else |w1|

    evaluated in float64 per point for both precisions, rounded once to the planes' real dtype; a point that
    falls back carries `phase_stft_gpu`'s value bit for bit (complex64: its float32 numerator and ``|Vg|^2``)."""
    lib = _lib.load()
    planes, (B, na, n), w = _five_planes('Vg', Vg, Vdg, Vddg, Vtg, Vtdg)
    sfs = to_device(np.ascontiguousarray(np.asarray(Sfs).reshape(-1)), w.dtype)
    if sfs.numel() != na:
        raise ValueError("`Sfs` must have one entry per row (%d != %d)" % (sfs.numel(), na))
    check(lib.ssq_stft2_phase(_CDT[w.dtype], *[_ptr(V) for V in planes], _ptr(sfs), _ptr(w), B, na, n,
                              float(gamma), float(chirp_tol), stream()))
    return w


def phase_cwt2_gpu(W, dW, Wd, dWd, dW3, scales, fs, gamma, chirp_tol=1e-3):
    """Second-order phase transform of the CWT (`ssq_cwt2_phase`, include/ssq_hip.h) from the planes
    ``Wx, dWx`` of the wavelet ``psih(w)``, ``Wx, dWx`` of ``psih'(w)`` and ``dWx`` of ``w psih(w)``
    (`wavelets.derived_wavelets`), each (na, n) or (B, na, n); `scales` (na,) in samples, ``r = scales / fs``::

        T   = -1j r Wd;  dT = -1j r dWd;  ddW = (1j / r) dW3
        den = W (W + dT) - T dW
        w1  = Im(dW / W) / 2pi
        w2  = w1 - Im((W ddW - dW^2) T / (den W)) / 2pi
        w   = inf where |W| < gamma else |w2| where |den| > chirp_tol |W|^2 else |w1|

    evaluated in float64 per point for both precisions, rounded once to the planes' real dtype; the infinities and
    the points that fall back are `phase_cwt_gpu`'s bit for bit (complex64: its float32 numerator and ``|W|^2``)."""
    lib = _lib.load()
    planes, (B, na, n), w = _five_planes('W', W, dW, Wd, dWd, dW3)
    sc = _row_vector('scales', scales, na, np.float64)      # a host array: the entry checks it
    check(lib.ssq_cwt2_phase(_CDT[w.dtype], *[_ptr(V) for V in planes], sc.ctypes.data, _ptr(w), B, na, n,
                             float(fs), float(gamma), float(chirp_tol), stream()))
    return w


def _conceft_call(entry, V, dV, row_values, proj, ssq_freqs, logscale, gamma, flipud, average, out):
    """The checks and the call `conceft_gpu` and `conceft_cwt_gpu` share. `row_values(rows, rdt)` gives the entry's
    per-row device vector: `Sfs` for `ssq_conceft`, the float64 weights for `ssq_conceft_cwt`."""
    if average not in ('abs', 'complex'):
        raise ValueError("`average` must be 'abs' or 'complex' (got %r)" % (average,))
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    lib = _lib.load()
    V, dV = list(V), list(dV)
    if not V or len(V) != len(dV):
        raise ValueError("`V` and `dV` must hold the same number of planes, at least one (got %d and %d)"
                         % (len(V), len(dV)))
    first = to_device(V[0])
    if first.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("the planes must be complex64 or complex128 (got %s)" % first.dtype)
    planes = [first] + [to_device(p, first.dtype) for p in V[1:] + dV]
    for p in planes[1:]:
        if p.shape != first.shape:
            raise ValueError("the planes must share one shape (got %s and %s)" % (tuple(first.shape), tuple(p.shape)))
    J = len(V)
    B, rows, n = _shape3(first)
    rdt = _real_of(first.dtype)
    rowv = row_values(rows, rdt)
    if hasattr(proj, 'detach'):
        proj = proj.detach().cpu().numpy()
    proj = np.asarray(proj, dtype=np.complex128)
    if proj.ndim != 2 or proj.shape[1] != J:
        raise ValueError("`proj` must be (Q, %d) (got %s)" % (J, proj.shape))
    r = np.ascontiguousarray(np.stack([proj.real, proj.imag], axis=-1))      # a host array: the entry checks it
    odt = rdt if average == 'abs' else first.dtype
    if out is None:
        out = torch.empty(first.shape, dtype=odt, device=first.device)
    else:
        _check_out(out, first, odt, "`out` must be a contiguous GPU tensor of the planes' shape, %s" % odt)
    kind, p = _grid(ssq_freqs, logscale)
    ptrs = ctypes.c_void_p * J
    check(getattr(lib, entry)(_CDT[first.dtype], ptrs(*[_ptr(t) for t in planes[:J]]),
                              ptrs(*[_ptr(t) for t in planes[J:]]), _ptr(rowv), r.ctypes.data, _ptr(out), B, J,
                              proj.shape[0], rows, n, float(gamma), kind, p, int(bool(flipud)),
                              int(average == 'complex'), stream()))
    return out


def conceft_gpu(V, dV, Sfs, proj, ssq_freqs, gamma, flipud=False, average='abs', out=None):
    """Multitaper synchrosqueezing in one kernel (`ssq_conceft`, include/ssq_hip.h states the definition; DESIGN.md
    4.5.5). `V`, `dV`: sequences of `J` complex planes, each (rows, n) or (B, rows, n) -- the STFTs of one signal with
    `J` orthonormal windows and with the windows' derivatives; `proj`: (Q, J) complex, used as given (`conceft_stft`
    normalises its rows); `Sfs`: (rows,); `ssq_freqs`: the linear grid the bins are taken on. Per projection `q` the
    planes are mixed, ``Vq = sum_j proj[q, j] V[j]``, `Vq` is reassigned by ``|Sfs - Im(dVq / Vq) / 2pi|`` where
    ``|Vq| >= gamma``, and the `Q` results are averaged: their magnitudes (``average='abs'``, a real array) or the
    complex values (``'complex'``). Float64 arithmetic for both precisions, rounded once; bit-reproducible."""
    def sfs(rows, rdt):
        vec = to_device(np.ascontiguousarray(np.asarray(Sfs).reshape(-1)), rdt)
        if vec.numel() != rows:
            raise ValueError("`Sfs` must have one entry per row (%d != %d)" % (vec.numel(), rows))
        return vec
    return _conceft_call('ssq_conceft', V, dV, sfs, proj, ssq_freqs, False, gamma, flipud, average, out)


def conceft_cwt_gpu(W, dW, proj, ssq_freqs, const, gamma, flipud=False, average='abs', out=None):
    """`conceft_gpu` for the CWT (`ssq_conceft_cwt`, include/ssq_hip.h). `W`, `dW`: sequences of `J`
    complex planes, each (rows, n) or (B, rows, n) -- the CWTs of one signal over `J` orthogonal wavelets and their time
    derivatives; `proj`: (Q, J) complex, used as given; `ssq_freqs`: (rows,), linear, 'log' or 'log-piecewise' (inferred
    from its values, as `ssqueeze` does); `const`: the rows' weights, a scalar or (rows,), sent as float64. Per
    projection `q` the planes are mixed, ``Wq = sum_j proj[q, j] W[j]``, ``Wq * const`` is reassigned by
    ``|Im(dWq / Wq)| / 2pi`` where ``|Wq| >= gamma``, and the `Q` results are averaged as `conceft_gpu` averages them.
    Float64 arithmetic for both precisions, rounded once; bit-reproducible."""
    from .scales import infer_scaletype
    if hasattr(ssq_freqs, 'detach'):
        ssq_freqs = ssq_freqs.detach().cpu().numpy()
    ssq_freqs = np.asarray(ssq_freqs)

    def weights(rows, rdt):
        c = const.detach().cpu().numpy() if hasattr(const, 'detach') else const
        c = np.asarray(c, dtype=np.float64).reshape(-1)
        if c.size not in (1, rows):
            raise ValueError("`const` must be a scalar or have one entry per row (%d != %d)" % (c.size, rows))
        return to_device(np.ascontiguousarray(np.broadcast_to(c, (rows,))), torch.float64)
    logscale = infer_scaletype(ssq_freqs)[0].startswith('log')
    return _conceft_call('ssq_conceft_cwt', W, dW, weights, proj, ssq_freqs, logscale, gamma, flipud, average, out)


_ROT_TABLES = {}


def default_dmax(n_fft, hop_len):
    """The largest displacement `time_reassign_gpu` keeps by default, in columns: half a window,
    ``ceil((n_fft // 2) / hop_len)`` -- a centre of gravity outside the window is no estimate."""
    return -(-(int(n_fft) // 2) // int(hop_len))


def rotation_table(n_fft):
    """``exp(-2j pi p / n_fft)``, ``p = 0 .. n_fft-1``, complex128 on the current device: NumPy's values, made once
    per (device, n_fft) -- `time_reassign_gpu`'s default `rot`."""
    key = (str(device()), int(n_fft))
    if key not in _ROT_TABLES:
        if len(_ROT_TABLES) >= 8:
            _ROT_TABLES.pop(next(iter(_ROT_TABLES)))
        _ROT_TABLES[key] = to_device(np.exp(-2j * np.pi * np.arange(int(n_fft)) / int(n_fft)))
    return _ROT_TABLES[key]


def time_reassign_gpu(Sx, Vtg, n_fft, hop_len, fs, gamma, rot=None, dmax=None, out=None):
    """Time-reassigned synchrosqueezing in one kernel (`ssq_time_reassign`, include/ssq_hip.h states the definition;
    DESIGN.md 4.5.7). `Sx`, `Vtg`: (rows, n) or (B, rows, n) complex -- the STFTs of one signal with the window `g` and
    with ``tau g``, `tau` the window's time axis in seconds (0 at the centre). Every point with ``|Sx| >= gamma`` moves
    along its row by ``d = rint(Re(Vtg / Sx) fs / hop_len)`` columns, if ``|d| <= dmax`` and the target is a column of
    the plane, and is added there as ``Sx[i, c] rot[(i c hop_len) mod n_fft]``, a cell's terms in ascending `c`.
    `rot`: None -> ``exp(-2j pi arange(n_fft) / n_fft)`` (cached per device and `n_fft`), False -> no rotation, or a
    ``(n_fft,)`` complex table of the caller's. `dmax`: None -> ``ceil((n_fft // 2) / hop_len)``. Float64 arithmetic
    for both precisions, rounded once; bit-reproducible."""
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    lib = _lib.load()
    Sx = to_device(Sx)
    if Sx.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`Sx` must be complex64 or complex128 (got %s)" % Sx.dtype)
    Vtg = to_device(Vtg, Sx.dtype)
    if Vtg.shape != Sx.shape:
        raise ValueError("`Sx` and `Vtg` must share one shape (got %s and %s)" % (tuple(Sx.shape), tuple(Vtg.shape)))
    B, rows, n = _shape3(Sx)
    n_fft, hop_len = int(n_fft), int(hop_len)
    if n_fft < 1 or hop_len < 1:
        raise ValueError("`n_fft` and `hop_len` must be >= 1 (got %d, %d)" % (n_fft, hop_len))
    if rot is None:
        rot = rotation_table(n_fft)
    elif rot is False:
        rot = None
    else:
        rot = to_device(rot, torch.complex128)
        if rot.shape != (n_fft,):
            raise ValueError("`rot` must be (n_fft,) = (%d,) (got %s)" % (n_fft, tuple(rot.shape)))
    if dmax is None:
        dmax = default_dmax(n_fft, hop_len)
    if out is None:
        out = torch.empty(Sx.shape, dtype=Sx.dtype, device=Sx.device)
    else:
        _check_out(out, Sx)
    check(lib.ssq_time_reassign(_CDT[Sx.dtype], _ptr(Sx), _ptr(Vtg), _ptr(rot), _ptr(out), B, rows, n, n_fft, hop_len,
                                float(fs) / hop_len, int(dmax), float(gamma), stream()))
    return out


def reassign2d_gpu(Sx, dSx, Vtg, n_fft, hop_len, fs, gamma, kmax=None, dmax=None, out=None, return_acc=False,
                   window=True):
    """The reassigned spectrogram in three launches (`ssq_reassign2d`, include/ssq_hip.h states the definition;
    DESIGN.md 4.5.9). `Sx`, `dSx`, `Vtg`: (rows, n) or (B, rows, n) complex -- the STFTs of one signal with the window
    `g`, with its derivative and with ``tau g``, `tau` the window's time axis in seconds (0 at the centre). The energy
    ``e = |Sx|^2`` of every point with ``|Sx| >= gamma`` moves by ``m = rint(-Im(dSx / Sx) / (2 pi) / (fs / n_fft))``
    rows, reflected at row 0, and by ``d = rint(Re(Vtg / Sx) fs / hop_len)`` columns, if ``|m| <= kmax``, ``|d| <=
    dmax`` and the target is a cell of the plane. ``dSx=None`` turns the frequency axis off (``m = 0``), ``Vtg=None``
    or ``dmax=0`` the time axis (``d = 0``). `kmax`: None -> ``rows - 1``; `dmax`: None -> ``ceil((n_fft // 2) /
    hop_len)``. Returns `Rx`, real, of `Sx`'s shape; with `return_acc` ``(Rx, acc, peak)``: the int64 fixed-point sums
    and, per signal, the bits of the largest kept energy.

    Float64 arithmetic for both precisions. A cell's sum is taken in fixed point -- every term is ``e 2^sh`` truncated to
    an integer, ``sh = 62 - bit_length(rows min(2 dmax + 1, n)) - frexp(max e)[1]`` per signal -- so it does not depend on
    the order of the additions: bit-reproducible, and below the exact sum by less than (the cell's terms) x ``2^-sh``,
    before the one rounding to the output's precision. ``window=False`` sends every term through a global atomic (the
    same bits, slower; for measurements)."""
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    lib = _lib.load()
    Sx, (dSx, Vtg), (B, rows, n) = _complex_planes('Sx', Sx, dSx=dSx, Vtg=Vtg)
    n_fft, hop_len = int(n_fft), int(hop_len)
    if n_fft < 1 or hop_len < 1:
        raise ValueError("`n_fft` and `hop_len` must be >= 1 (got %d, %d)" % (n_fft, hop_len))
    if dmax is None:
        dmax = default_dmax(n_fft, hop_len)
    if Vtg is None:
        dmax = 0
    if kmax is None:
        kmax = rows - 1
    rdt = _real_of(Sx.dtype)
    if out is None:
        out = torch.empty(Sx.shape, dtype=rdt, device=Sx.device)
    else:
        _check_out(out, Sx, rdt, "`out` must be a contiguous real GPU tensor of `Sx`'s shape and precision")
    acc, peak = _fixed_point_buffers(Sx, B)
    flags = (_lib.REASSIGN2D_FREQ if dSx is not None else 0) | (0 if window else _lib.REASSIGN2D_NO_WINDOW)
    check(lib.ssq_reassign2d(_CDT[Sx.dtype], _ptr(Sx), _ptr(dSx), _ptr(Vtg), _ptr(out), _ptr(acc), _ptr(peak), B, rows, n,
                             n_fft, hop_len, float(fs), float(fs) / hop_len, int(kmax), int(dmax), float(gamma), flags,
                             stream()))
    return (out, acc, peak) if return_acc else out


TSSQ_MAX_DMAX = 1 << 20        # ssq_time_reassign_max_dmax(): the largest displacement the reassignment entries accept


def reassign_cwt_dmax(scales, time_std, max_shift=4.):
    """The largest displacement `reassign_cwt_gpu` keeps per row, in columns, int32: ``min(ceil(max_shift time_std
    scales[i]), 2^20)`` -- `time_std` the standard deviation of ``|psi(t)|^2`` at scale 1 in samples
    (`wavelets.wavelet_time_std`), `scales` in samples. A centre of gravity further out than a few standard deviations
    of the wavelet is no estimate: ``Re(T / W)`` of a noise-dominated point is Cauchy-like."""
    if not (np.isfinite(max_shift) and max_shift >= 0 and np.isfinite(time_std) and time_std >= 0):
        raise ValueError("`max_shift` and `time_std` must be finite and >= 0 (got %r, %r)" % (max_shift, time_std))
    sc = np.asarray(scales, dtype=np.float64).reshape(-1)
    return np.minimum(np.ceil(float(max_shift) * float(time_std) * sc), TSSQ_MAX_DMAX).astype(np.int32)


def _host_bins(w, kind, p, omax):
    """`bin_from_w` (csrc/ssq_point_math.inl) for a host vector of positive finite frequencies, before `flipud`."""
    w = np.asarray(w, dtype=np.float64)
    p = [float(v) for v in p]
    if kind == _lib.GRID_LIN:
        t = (w - p[0]) / p[1]
    elif kind == _lib.GRID_LOG:
        t = (np.log2(w) - p[0]) / p[1]
    else:
        wl = np.log2(w)
        t = np.where(wl > p[1], (wl - p[1]) / p[3] + np.trunc(p[4]), (wl - p[0]) / p[2])
    return np.clip(np.rint(t), 0, omax).astype(np.int32)


def reassign_cwt_home(scales, ssq_freqs, flipud=False, freq=True, wc=None, fs=1.):
    """`reassign_cwt_gpu`'s default `home`: per row the bin of its own centre frequency, ``wc fs / (2 pi scales[i])``
    with `wc` the wavelet's peak radian frequency at scale 1 (`wavelets.center_frequency`, ``kind='peak-ct'``), after
    `flipud`; the row itself with the frequency axis off. Without `wc` the centre frequency is taken as the grid's top
    frequency times ``scales.min() / scales[i]``, which is how `ssq_cwt` lays its grid out (``maprange='peak'``) up to
    the clip at Nyquist. int32, host."""
    from .scales import infer_scaletype
    from .ssqueezing import ssq_grid_params
    sc = np.asarray(scales, dtype=np.float64).reshape(-1)
    if not freq:
        return np.arange(sc.size, dtype=np.int32)
    v = np.asarray(ssq_freqs, dtype=np.float64).reshape(-1)
    kind, p = ssq_grid_params(v, v.size > 2 and infer_scaletype(v)[0].startswith('log'))
    fc = v.max() * sc.min() / sc if wc is None else float(wc) * float(fs) / (2 * np.pi * sc)
    k = _host_bins(fc, kind, p, sc.size - 1)
    return (sc.size - 1 - k).astype(np.int32) if flipud else k


def reassign_cwt_gpu(W, dW, Wd, scales, cst, dmax, ssq_freqs, gamma, flipud=False, out=None, return_acc=False,
                     window=True, home=None):
    """The reassigned scalogram in three launches (`ssq_reassign_cwt`, include/ssq_hip.h states the definition;
    DESIGN.md 4.5.10): the CWT counterpart of `reassign2d_gpu`. `W`, `dW`, `Wd`: (rows, n) or (B, rows, n) complex --
    the CWT of one signal over ``psih(w)``, its time derivative, and the CWT over ``psih'(w)``
    (`wavelets.derived_wavelets`); `scales` (rows,) in samples; `cst` the rows' weights, a scalar or (rows,), sent as
    float64; `dmax` (rows,) integers, the largest displacement kept per row (`reassign_cwt_dmax`); `ssq_freqs` (rows,),
    linear, 'log' or 'log-piecewise' (inferred from its values, as `ssqueeze` does). The weighted energy
    ``|W|^2 cst[i]`` of every point with ``|W| >= gamma`` moves to the bin of ``|Im(dW / W)| / 2pi`` on the grid
    (`flipud`: mirrored) and by ``d = rint(Im(Wd / W) scales[i])`` columns -- ``Re(T / W)`` with ``T = -1j r Wd`` -- if
    ``|d| <= dmax[i]`` and the target is a column of the plane. ``dW=None`` turns the frequency axis off (a point stays in
    its row; `ssq_freqs` may be None), ``Wd=None`` the time axis (`dmax` may be None). Returns `Rx`, real, of `W`'s
    shape; with `return_acc` ``(Rx, acc, peak)``: the int64 fixed-point sums and, per signal, the bits of the largest
    kept term.

    Float64 arithmetic for both precisions; the sum is `reassign2d_gpu`'s fixed-point sum with ``C = sum_i min(2 dmax[i]
    + 1, n)`` (``max_i`` with the frequency axis off), so the result is bit-reproducible and below the exact sum by less
    than (the cell's terms) x ``2^-sh``. `home` (rows,) integers: where the energy of row `i` is expected to land
    (None: `reassign_cwt_home`); it places the LDS windows and affects speed only, as does ``window=False`` (every term
    through a global atomic)."""
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    lib = _lib.load()
    W, (dW, Wd), (B, rows, n) = _complex_planes('W', W, dW=dW, Wd=Wd)
    freq, time = dW is not None, Wd is not None
    c = _row_vector('cst', cst, rows, np.float64, scalar_ok=True)
    if not (np.isfinite(c).all() and (c >= 0).all()):
        raise ValueError("`cst` must be finite and >= 0")
    sc = _row_vector('scales', scales, rows, np.float64)
    dm = _row_dmax(dmax, rows) if time else None
    kind, p = 0, None
    if freq:
        from .scales import infer_scaletype
        ssq_freqs = _row_vector('ssq_freqs', ssq_freqs, rows)
        # (two values are evenly spaced in any metric: they are taken as a linear grid)
        kind, p = _grid(ssq_freqs, rows > 2 and infer_scaletype(ssq_freqs)[0].startswith('log'))
    if home is None:
        home = reassign_cwt_home(sc, ssq_freqs, flipud, freq)
    else:
        home = np.clip(_row_vector('home', home, rows, np.int64), np.iinfo(np.int32).min,
                       np.iinfo(np.int32).max).astype(np.int32)
    rdt = _real_of(W.dtype)
    if out is None:
        out = torch.empty(W.shape, dtype=rdt, device=W.device)
    else:
        _check_out(out, W, rdt, "`out` must be a contiguous real GPU tensor of `W`'s shape and precision")
    acc, peak = _fixed_point_buffers(W, B)
    cst_d, rsc_d = to_device(c), to_device(sc)
    home_d = to_device(np.ascontiguousarray(home))
    flags = ((_lib.REASSIGN_CWT_FREQ if freq else 0) | (_lib.REASSIGN_CWT_TIME if time else 0)
             | (0 if window else _lib.REASSIGN_CWT_NO_WINDOW))
    check(lib.ssq_reassign_cwt(_CDT[W.dtype], _ptr(W), _ptr(dW), _ptr(Wd), _ptr(cst_d), _ptr(rsc_d),
                               dm.ctypes.data if time else None, _ptr(home_d), _ptr(out), _ptr(acc), _ptr(peak), B, rows,
                               n, float(gamma), kind, p, int(bool(flipud)), flags, stream()))
    return (out, acc, peak) if return_acc else out


_CWT_ROT_TABLES = {}


def _exact_turns(freqs, mult, count):
    """``frac(freqs[i] * mult * k)`` for ``k = 0 .. count-1``, float64 (rows, count): the fractional part of the exact
    product, every frequency taken as the float64 it is (a ratio of Python integers), rounded once at the end."""
    out = np.empty((len(freqs), count), dtype=np.float64)
    for i, f in enumerate(freqs):
        num, den = float(f).as_integer_ratio()
        num *= int(mult)
        out[i] = [((num * k) % den) / den for k in range(count)]
    return out


def cwt_rotation_tables(row_freqs, n, fs=1.):
    """``(rot_lo, rot_hi)``, complex128 on the current device: the two-level table of `time_reassign_cwt_gpu`'s rotation
    ``rot(i, c) = exp(-2j pi phi_i c) = rot_hi[i, c // P] rot_lo[i, c % P]`` with ``phi_i = row_freqs[i] / fs`` cycles
    per column and ``P = 256``: ``rot_lo`` is (rows, P), ``rot_hi`` (rows, ceil(n / P)), and an entry is ``exp(-2j pi
    frac)`` with `frac` the exact fractional part of ``phi_i p`` (``phi_i P q``), `phi_i` taken as the float64 it is.
    ``phi_i`` is not rational in `n`, so no table indexed ``mod n`` serves, and a direct ``exp(-2j pi phi c)`` loses
    ``c eps`` of a turn; the product of two exactly reduced entries stays within a few ulp. `row_freqs`:
    `wavelets.row_frequencies`; must be finite and positive. Cached per content (the eight most recent)."""
    f = row_freqs.detach().cpu().numpy() if hasattr(row_freqs, 'detach') else row_freqs
    f = np.ascontiguousarray(np.asarray(f, dtype=np.float64).reshape(-1))
    fs, n = float(fs), int(n)
    if n < 1:
        raise ValueError("`n` must be >= 1 (got %d)" % n)
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("`fs` must be finite and positive (got %r)" % (fs,))
    phi = f / fs
    if f.size < 1 or not (np.isfinite(phi).all() and (phi > 0).all()):
        raise ValueError("`row_freqs` must be finite and positive")
    P = _lib.TSSQ_CWT_ROT_P
    nq = -(-n // P)
    key = (str(device()), phi.tobytes(), nq)
    if key not in _CWT_ROT_TABLES:
        if len(_CWT_ROT_TABLES) >= 8:
            _CWT_ROT_TABLES.pop(next(iter(_CWT_ROT_TABLES)))
        lo, hi = _exact_turns(phi, 1, P), _exact_turns(phi, P, nq)
        _CWT_ROT_TABLES[key] = (to_device(np.exp(-2j * np.pi * lo)), to_device(np.exp(-2j * np.pi * hi)))
    return _CWT_ROT_TABLES[key]


def time_reassign_cwt_shift(emax, dmax, n):
    """`sh` of `time_reassign_cwt_gpu`'s fixed-point sum for one signal, as the entry takes it: ``61 - bit_length(max_i
    min(2 dmax[i] + 1, n)) - ceil(frexp(emax)[1] / 2)``, `emax` the largest kept ``|W|^2`` (the float64 whose bits
    `return_acc` hands back as `peak`). ``ldexp(acc, -sh)`` is the sum `acc` stands for; a term is within ``2^-sh`` of its
    value per component."""
    dm = np.asarray(dmax, dtype=np.int64).reshape(-1)
    C = int(np.minimum(2 * dm + 1, int(n)).max())
    ex = int(np.frexp(np.float64(emax))[1])
    return 61 - C.bit_length() + (-ex) // 2


def time_reassign_cwt_gpu(W, Wd, scales, dmax, gamma, rot=None, out=None, return_acc=False, window=True):
    """The time-reassigned synchrosqueezed CWT in three launches (`ssq_time_reassign_cwt`, include/ssq_hip.h states the
    definition): the CWT counterpart of `time_reassign_gpu`. `W`, `Wd`: (rows, n) or (B, rows, n)
    complex -- the CWT of one signal over ``psih(w)`` and over ``psih'(w)`` (`wavelets.derived_wavelets`); `scales`
    (rows,) in samples; `dmax` (rows,) integers, the largest displacement kept per row (`reassign_cwt_dmax`). Every point
    with ``|W| >= gamma`` moves along its row by ``d = rint(Im(Wd / W) scales[i])`` columns, if ``|d| <= dmax[i]`` and the
    target is a column of the plane, and is added there as ``W[i, c] rot(i, c)``. `rot`: the ``(rot_lo, rot_hi)`` pair
    of `cwt_rotation_tables` for the rows' frequencies, or False for no rotation; None is refused -- the kernel cannot
    know the rows' frequencies. Returns `Tx`, complex, of `W`'s shape; with `return_acc` ``(Tx, acc, peak)``: the int64
    fixed-point sums, ``W.shape + (2,)``, and, per signal, the bits of the largest kept ``|W|^2``.

    Float64 arithmetic for both precisions. A cell's sum is taken in signed fixed point, real and imaginary parts
    apart: a term's component is scaled by ``2^sh`` and truncated toward zero, ``sh = 61 - bit_length(max_i min(2
    dmax[i] + 1, n)) - ceil(frexp(max |W|^2)[1] / 2)`` per signal, so the result does not depend on the order of the
    additions: bit-reproducible, and within (the cell's terms) x ``2^-sh`` of the exact sum per component, before the
    one rounding to the output's precision. ``window=False`` sends every term through global atomics (the same bits;
    for measurements)."""
    if gamma is None:
        raise ValueError("`gamma` must not be None")
    if rot is None:
        raise ValueError("`rot` must be the (rot_lo, rot_hi) pair of `cwt_rotation_tables` for the rows' frequencies, "
                         "or False for no rotation: the kernel cannot know them")
    lib = _lib.load()
    W, (Wd,), (B, rows, n) = _complex_planes('W', W, Wd=to_device(Wd))     # (`Wd` is not optional: None raises)
    sc = _row_vector('scales', scales, rows, np.float64)
    dm = _row_dmax(dmax, rows)
    lo = hi = None
    if rot is not False:
        try:
            lo, hi = rot
        except (TypeError, ValueError):
            raise ValueError("`rot` must be a (rot_lo, rot_hi) pair (`cwt_rotation_tables`) or False")
        lo, hi = to_device(lo, torch.complex128), to_device(hi, torch.complex128)
        P = _lib.TSSQ_CWT_ROT_P
        if lo.shape != (rows, P) or hi.shape != (rows, -(-n // P)):
            raise ValueError("`rot` must be (rows, %d) and (rows, ceil(n / %d)) = (%d, %d) (got %s and %s)"
                             % (P, P, rows, -(-n // P), tuple(lo.shape), tuple(hi.shape)))
    if out is None:
        out = torch.empty(W.shape, dtype=W.dtype, device=W.device)
    else:
        _check_out(out, W)
    acc, peak = _fixed_point_buffers(W, B, words=2)
    rsc_d = to_device(sc)
    check(lib.ssq_time_reassign_cwt(_CDT[W.dtype], _ptr(W), _ptr(Wd), _ptr(rsc_d), dm.ctypes.data, _ptr(lo), _ptr(hi),
                                    _ptr(out), _ptr(acc), _ptr(peak), B, rows, n, float(gamma),
                                    0 if window else _lib.TSSQ_CWT_NO_WINDOW, stream()))
    return (out, acc, peak) if return_acc else out


def _linear_grid(name, v):
    """`v` as a float64 host vector of two or more evenly spaced values (`name` in the message)."""
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    eps = np.finfo(v.dtype).eps if v.dtype.kind == 'f' else np.finfo(np.float64).eps
    v = v.astype(np.float64).reshape(-1)
    if v.size < 2:
        raise ValueError("`%s` must hold two values or more (got %d)" % (name, v.size))
    step = v[1] - v[0]
    if not np.all(np.abs(v - (v[0] + step * np.arange(v.size))) <= 1e3 * eps * np.abs(v).max()):
        raise ValueError("`%s` must be linearly distributed" % name)
    return v


def multi_squeeze_gpu(Sx, w, Sfs, ssq_freqs, const=1, n_iter=10, interp='linear', flipud=False, out=None, get_w=False):
    """Multisynchrosqueezing in one kernel (`ssq_multi_squeeze`, include/ssq_hip.h states the definition; DESIGN.md
    4.5.8). `Sx`: (rows, n) or (B, rows, n) complex; `w`: its phase transform (`phase_stft_gpu`, `phase_stft2_gpu`;
    ``inf`` = skip), same shape; `Sfs`: (rows,), linear -- row `i` sits at ``f0 + i df``, ``f0 = Sfs[0]``, ``df =
    Sfs[1] - Sfs[0]`` in float64; `ssq_freqs`: (rows,), the linear grid the bins are taken on; `const` as
    `indexed_sum_onfly`'s. Per column, every point's frequency ``f = w[i]`` is replaced ``n_iter - 1`` times by `w`
    at the row `f` points to -- interpolated between the two neighbouring rows (``interp='linear'``) or taken from
    the nearest (``'nearest'``, the paper's form) --, stopping at a fixed point, outside the rows' range or in front
    of an ``inf``; the point is then added to the bin of its final frequency, a cell's terms in ascending row order.
    ``n_iter=1`` is `indexed_sum_onfly`. The iteration runs in float64 for both precisions, the final frequency is
    rounded once; bit-reproducible. Returns `Tx`, or ``(Tx, w_final)`` with `get_w`."""
    if interp not in ('linear', 'nearest'):
        raise ValueError("`interp` must be 'linear' or 'nearest' (got %r)" % (interp,))
    lib = _lib.load()
    Sx = to_device(Sx)
    if Sx.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`Sx` must be complex64 or complex128 (got %s)" % Sx.dtype)
    w = to_device(w, _real_of(Sx.dtype))
    if Sx.shape != w.shape:
        raise ValueError("`Sx` and `w` shapes differ")
    B, rows, n = _shape3(Sx)
    sfs, grid = _linear_grid('Sfs', Sfs), _linear_grid('ssq_freqs', ssq_freqs)
    if sfs.size != rows or grid.size != rows:
        raise ValueError("`Sfs` and `ssq_freqs` must have one entry per row (%d, %d != %d)" % (sfs.size, grid.size, rows))
    if out is None:
        out = torch.empty_like(Sx)
    else:
        _check_out(out, Sx)
    wf = torch.empty_like(w) if get_w else None
    cst, c64 = _const_vector(const, rows, Sx.dtype)
    kind, p = _grid(ssq_freqs, False)
    check(lib.ssq_multi_squeeze(_CDT[Sx.dtype], _ptr(Sx), _ptr(w), _ptr(out), _ptr(wf), _ptr(cst), c64, B, rows, n,
                                float(sfs[0]), float(sfs[1] - sfs[0]), int(n_iter), int(interp == 'linear'), kind, p,
                                int(bool(flipud)), stream()))
    return (out, wf) if get_w else out


def _row_table(name, v, rows):
    """`v` as a contiguous float64 host vector of `rows` finite, strictly monotone values (`name` in the message)."""
    v = _row_vector(name, v, rows, np.float64)
    if not np.isfinite(v).all():
        raise ValueError("`%s` must be finite" % name)
    d = np.diff(v)
    if not ((d > 0).all() or (d < 0).all()):
        raise ValueError("`%s` must be strictly monotone" % name)
    return v


def multi_squeeze_cwt_gpu(Wx, w, row_freqs, ssq_freqs, const=1, n_iter=10, interp='linear', flipud=False, out=None,
                          get_w=False):
    """Multisynchrosqueezing on a table of rows in one kernel (`ssq_multi_squeeze_cwt`, include/ssq_hip.h states the
    definition): `multi_squeeze_gpu` for the CWT. `Wx`: (rows, n) or (B, rows, n) complex; `w`: its
    phase transform (`phase_cwt_gpu`, `phase_cwt2_gpu`; ``inf`` = skip), same shape; `row_freqs`: (rows,), the rows'
    centre frequencies (`wavelets.row_frequencies`), finite and strictly monotone in either direction, sent as float64;
    `ssq_freqs`: (rows,), the grid the bins are taken on -- linear, 'log' or 'log-piecewise' (inferred from its values,
    as `reassign_cwt_gpu` does); `const` as `indexed_sum_onfly`'s. Per column, every point's frequency ``f = w[i]`` is
    replaced ``n_iter - 1`` times by `w` at the place `f` takes between two rows of the table -- interpolated between
    them (``interp='linear'``) or taken from the nearer (``'nearest'``) --, stopping at a fixed point, outside the
    table's range or in front of an ``inf``; the point is then added to the bin of its final frequency, a cell's terms
    in ascending row order. ``n_iter=1`` is `indexed_sum_onfly`. The iteration runs in float64 for both precisions,
    the final frequency is rounded once; bit-reproducible. Returns `Tx`, or ``(Tx, w_final)`` with `get_w`."""
    if interp not in ('linear', 'nearest'):
        raise ValueError("`interp` must be 'linear' or 'nearest' (got %r)" % (interp,))
    from .scales import infer_scaletype
    lib = _lib.load()
    Wx = to_device(Wx)
    if Wx.dtype not in (torch.complex64, torch.complex128):
        raise TypeError("`Wx` must be complex64 or complex128 (got %s)" % Wx.dtype)
    w = to_device(w, _real_of(Wx.dtype))
    if Wx.shape != w.shape:
        raise ValueError("`Wx` and `w` shapes differ")
    B, rows, n = _shape3(Wx)
    fr = _row_table('row_freqs', row_freqs, rows)
    ssq_freqs = _row_vector('ssq_freqs', ssq_freqs, rows)
    # (two values are evenly spaced in any metric: they are taken as a linear grid)
    kind, p = _grid(ssq_freqs, rows > 2 and infer_scaletype(ssq_freqs)[0].startswith('log'))
    if out is None:
        out = torch.empty_like(Wx)
    else:
        _check_out(out, Wx)
    wf = torch.empty_like(w) if get_w else None
    cst, c64 = _const_vector(const, rows, Wx.dtype)
    check(lib.ssq_multi_squeeze_cwt(_CDT[Wx.dtype], _ptr(Wx), _ptr(w), _ptr(out), _ptr(wf), _ptr(cst), c64,
                                    fr.ctypes.data, B, rows, n, int(n_iter), int(interp == 'linear'), kind, p,
                                    int(bool(flipud)), stream()))
    return (out, wf) if get_w else out


def replace_under_abs(x, ref=None, value=1., replacement=0., parallel=None):
    """In place: ``x[abs(ref) < value] = replacement`` (`ref` complex, `x` real GPU
    tensors). Reference: `replace_under_abs`, ssqueezepy/algos.py:498-579."""
    lib = _lib.load()
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise TypeError("`x` must be a GPU tensor (modified in place)")
    ref = to_device(ref)
    if ref.dtype not in (torch.complex64, torch.complex128):
        ref = ref.to(torch.complex64 if x.dtype == torch.float32 else
                     torch.complex128)
    if x.dtype != _real_of(ref.dtype) or not x.is_contiguous():
        raise TypeError("`x` must be contiguous and of `ref`'s real dtype")
    check(lib.ssq_replace_under_abs(_CDT[ref.dtype], _ptr(x), _ptr(ref), x.numel(),
                                    float(value), float(replacement), stream()))
    return x


def buffer(x, seg_len, n_overlap, modulated=False, parallel=None):
    """Frames of `x` as columns: ``(seg_len, n_segs)`` or batched
    ``(B, seg_len, n_segs)``. Reference: `buffer`, utils/stft_utils.py:20-66."""
    lib = _lib.load()
    x = to_device(x)
    assert x.ndim in (1, 2)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    hop = seg_len - n_overlap
    n_x = x.shape[-1]
    n_segs = (n_x - seg_len) // hop + 1
    B = 1 if x.ndim == 1 else x.shape[0]
    out = torch.empty((B, seg_len, n_segs), dtype=x.dtype, device=x.device)
    check(lib.ssq_buffer(_CDT[x.dtype], _ptr(x), _ptr(out), B, n_x, seg_len,
                         n_overlap, int(bool(modulated)), stream()))
    return out[0] if x.ndim == 1 else out


def pad_signal_gpu(x, n1, n2, padtype='reflect'):
    """Device signal extension (the kernel behind `cwt`/`stft` padding)."""
    lib = _lib.load()
    x = to_device(x)
    B = 1 if x.ndim == 1 else x.shape[0]
    n = x.shape[-1]
    out = torch.empty((B, n1 + n + n2), dtype=x.dtype, device=x.device)
    check(lib.ssq_pad_signal(_CDT[x.dtype], _ptr(x), _ptr(out), B, n, n1, n2,
                             _lib.PAD[padtype], stream()))
    return out[0] if x.ndim == 1 else out


# ------------------------------------------------------------------ inverses
def wants_grad(x):
    """Whether a function of `x` is to carry a gradient: a tensor that requires one, with grad
    mode on."""
    return isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled()


def _divisor(divisor, na, rdt):
    if divisor is None:
        return None
    d = to_device(np.ascontiguousarray(np.asarray(divisor).reshape(-1)), rdt)
    if d.numel() != na:
        raise ValueError("`divisor` must have one entry per row (%d != %d)"
                         % (d.numel(), na))
    return d


def _colsum(Z, d):
    B, na, n = _shape3(Z)
    out = torch.empty(Z.shape[:-2] + (n,), dtype=_real_of(Z.dtype), device=Z.device)
    check(_lib.load().ssq_colsum(_CDT[Z.dtype], _ptr(Z), _ptr(d), _ptr(out), B, na, n,
                                 stream()))
    return out


def colsum_adjoint(g, na, divisor=None):
    """Adjoint of `colsum_real`: ``gZ[..., i, j] = g[..., j] [/ divisor[i]] + 0j`` (`ssq_colsum_adjoint`);
    `g` real (n,) or (B, n), `gZ` complex (na, n) or (B, na, n) of the matching precision."""
    g = to_device(g).contiguous()
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError("`g` must be float32 or float64 (got %s)" % g.dtype)
    d = divisor if isinstance(divisor, torch.Tensor) else _divisor(divisor, na, g.dtype)
    n = g.shape[-1]
    B = 1 if g.ndim == 1 else g.shape[0]
    cdt = torch.complex64 if g.dtype == torch.float32 else torch.complex128
    gZ = torch.empty(g.shape[:-1] + (int(na), n), dtype=cdt, device=g.device)
    check(_lib.load().ssq_colsum_adjoint(_CDT[g.dtype], _ptr(g), _ptr(d), _ptr(gZ), B, int(na), n,
                                         stream()))
    return gZ


class _ColsumFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, d):
        ctx.d, ctx.na = d, Z.shape[-2]
        return _colsum(Z.detach(), d)

    @staticmethod
    def backward(ctx, g):
        return colsum_adjoint(g, ctx.na, ctx.d), None


def colsum_real(Z, divisor=None):
    """``sum_i Re(Z[..., i, :]) [/ divisor[i]]`` over the scale / frequency axis, rows in
    ascending order in `Z`'s own precision (bit-identical to NumPy's
    ``(Z.real / d).sum(axis=-2)``). `Z`: (na, n) or (B, na, n) complex. Differentiable w.r.t. `Z`
    (`colsum_adjoint`)."""
    grad = wants_grad(Z)
    Z = to_device(Z)
    B, na, n = _shape3(Z)
    d = _divisor(divisor, na, _real_of(Z.dtype))
    return _ColsumFunction.apply(Z, d) if grad else _colsum(Z.detach(), d)


def _bands(lo, hi, Z):
    """`lo`, `hi` (K, n) or (B, K, n) as int32 device arrays, and whether every signal has its own."""
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    hi = np.ascontiguousarray(hi, dtype=np.int32)
    if lo.shape != hi.shape or lo.ndim not in (2, 3) or lo.shape[-1] != Z.shape[-1]:
        raise ValueError("`lo`, `hi` must be (K, n) or (B, K, n) (got %s, %s; n = %d)"
                         % (lo.shape, hi.shape, Z.shape[-1]))
    if lo.ndim == 3 and (Z.ndim != 3 or lo.shape[0] != Z.shape[0]):
        raise ValueError("per-signal bands %s do not match a transform of shape %s"
                         % (lo.shape, tuple(Z.shape)))
    return (torch.as_tensor(lo, device=Z.device), torch.as_tensor(hi, device=Z.device),
            lo.ndim == 3)


def _band_colsum(Z, lo, hi, own):
    B, na, n = _shape3(Z)
    K = lo.shape[-2]
    out = torch.empty(Z.shape[:-2] + (K + 1, n), dtype=torch.float64, device=Z.device)
    check(_lib.load().ssq_band_colsum_batch(_CDT[Z.dtype], _ptr(Z), _ptr(lo), _ptr(hi), int(own), K,
                                            _ptr(out), B, na, n, stream()))
    return out


def band_colsum_adjoint(g, lo, hi, na, cdtype):
    """Adjoint of `band_colsum`: ``gZ[..., i, j]`` = the sum, bands ascending, of ``g[..., k, j]`` over
    the bands that hold row `i` -- ``g[..., K, j]`` where none does -- in float64, rounded once to
    `cdtype`; imaginary part zero (`ssq_band_colsum_adjoint`)."""
    g = to_device(g, torch.float64)
    gZ = torch.empty(g.shape[:-2] + (int(na), g.shape[-1]), dtype=cdtype, device=g.device)
    if not isinstance(lo, torch.Tensor):
        lo, hi, own = _bands(lo, hi, gZ)
    else:
        own = lo.ndim == 3
    B, _, n = _shape3(gZ)
    check(_lib.load().ssq_band_colsum_adjoint(_CDT[cdtype], _ptr(g), _ptr(lo), _ptr(hi), int(own),
                                              lo.shape[-2], _ptr(gZ), B, int(na), n, stream()))
    return gZ


class _BandColsumFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, lo, hi, own):
        ctx.lo, ctx.hi, ctx.na, ctx.cdt = lo, hi, Z.shape[-2], Z.dtype
        return _band_colsum(Z.detach(), lo, hi, own)

    @staticmethod
    def backward(ctx, g):
        return band_colsum_adjoint(g, ctx.lo, ctx.hi, ctx.na, ctx.cdt), None, None, None


def band_colsum(Z, lo, hi):
    """Per-component sums of ``Re(Z)`` over the row bands ``lo[k, j] .. hi[k, j]`` of every
    column (float64), plus the sum of the rows no band covers as the last row.
    `Z`: (na, n) or (B, na, n) complex; `lo`, `hi`: (K, n) integer arrays, inclusive, shared by
    the signals, or (B, K, n). Differentiable w.r.t. `Z` (`band_colsum_adjoint`)."""
    grad = wants_grad(Z)
    Z = to_device(Z)
    _shape3(Z)
    lo, hi, own = _bands(lo, hi, Z)
    if grad:
        return _BandColsumFunction.apply(Z, lo, hi, own)
    return _band_colsum(Z.detach(), lo, hi, own)


def istft_algo(dtype, n_fft, n_hops, hop_len, N):
    """The route `istft_gpu` and its backward take for a shape: 'fused' or 'rocfft' (`ssq_istft_algo`)."""
    code = F32 if str(dtype) in ('float32', 'torch.float32', 'torch.complex64', 'complex64') else F64
    return _lib.load().ssq_istft_algo(code, int(n_fft), int(n_hops), int(hop_len), int(N)).decode()


def _istft(Sx, wa, wa1, n_fft, hop_len, N, modulated):
    B, rows, n_hops = _shape3(Sx)
    x = torch.empty(Sx.shape[:-2] + (int(N),), dtype=_real_of(Sx.dtype), device=Sx.device)
    check(_lib.load().ssq_istft_batch(_CDT[Sx.dtype], _ptr(Sx), _ptr(wa), _ptr(wa1), _ptr(x), B,
                                      int(n_fft), int(n_hops), int(hop_len), int(N),
                                      int(bool(modulated)), stream()))
    return x


def istft_adjoint_gpu(g, win_a, win_a1, n_fft, n_hops, hop_len, modulated=True):
    """Adjoint of `istft_gpu`: `g` real (N,) or (B, N) -> `gSx` complex (n_fft//2 + 1, n_hops) or
    batched (`ssq_istft_adjoint`, include/ssq_hip.h states the formula)."""
    g = to_device(g).contiguous()
    rdt = g.dtype
    cdt = torch.complex64 if rdt == torch.float32 else torch.complex128
    wa, wa1 = to_device(win_a, rdt), to_device(win_a1, rdt)
    B = 1 if g.ndim == 1 else g.shape[0]
    N = g.shape[-1]
    gSx = torch.empty(g.shape[:-1] + (int(n_fft) // 2 + 1, int(n_hops)), dtype=cdt, device=g.device)
    check(_lib.load().ssq_istft_adjoint(_CDT[rdt], _ptr(g), _ptr(wa), _ptr(wa1), _ptr(gSx), B,
                                        int(n_fft), int(n_hops), int(hop_len), int(N),
                                        int(bool(modulated)), stream()))
    return gSx


class _IstftFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Sx, wa, wa1, n_fft, hop_len, N, modulated):
        ctx.args = (wa, wa1, n_fft, Sx.shape[-1], hop_len, modulated)
        return _istft(Sx.detach(), wa, wa1, n_fft, hop_len, N, modulated)

    @staticmethod
    def backward(ctx, g):
        return (istft_adjoint_gpu(g, *ctx.args),) + (None,) * 6


def istft_gpu(Sx, win_a, win_a1, n_fft, hop_len, N, modulated=True):
    """irfft of every column of `Sx` + overlap-add with `win_a`, divided by the
    overlap-added `win_a1`, trimmed to `N` samples (`ssq_istft_batch`, include/ssq_hip.h).
    `Sx`: (n_fft//2 + 1, n_hops) or (B, n_fft//2 + 1, n_hops). Differentiable w.r.t. `Sx`
    (`istft_adjoint_gpu`)."""
    grad = wants_grad(Sx)
    Sx = to_device(Sx)
    B, rows, n_hops = _shape3(Sx)
    if rows != int(n_fft) // 2 + 1:
        raise ValueError("`Sx` has %d rows, n_fft = %d needs %d" % (rows, n_fft, int(n_fft) // 2 + 1))
    rdt = _real_of(Sx.dtype)
    wa, wa1 = to_device(win_a, rdt), to_device(win_a1, rdt)
    if grad:
        return _IstftFunction.apply(Sx, wa, wa1, int(n_fft), int(hop_len), int(N), bool(modulated))
    return _istft(Sx.detach(), wa, wa1, n_fft, hop_len, N, modulated)
