# -*- coding: utf-8 -*-
"""Shared by the tests of the fused float32 STFT BY WINDOW LENGTH (test_gpu_stft_lengths.py on the device,
test_stft_lengths_emulated.py under the CPU emulator, test_stft_lengths_design.py on the host alone): the table of
lengths with what each is there for, a Python restatement of the mixed-radix kernel's planning rule, the NumPy
float64 statement of `stft` with its derivative, and the per-column check.

The mixed-radix kernel (csrc/ssq_stft_generic.hip) runs one Stockham pass per factor of `n_fft` -- 16s, 8s, 4s, a 2,
then the odd primes 3 .. 31 ascending -- on G frames per workgroup. A pass has two arms: the first (`Ns == 1`: no
twiddles, no division) and every later one (`Ns > 1`: `j / Ns` by a multiply-high, twiddle stride `k * tstep`, output
stride `Ns << lgG`). What selects a code path is therefore the POSITION of a radix (first, middle, last, alone), G
(16, 8, 4, 2, 1: the `lgG` shifts, and how many epilogue points a work-item holds) and the grid (the remap per XCD from
64 workgroups on). `LENGTHS` puts every radix into every position it can take below 4992, a length on both sides of
every G edge, and the lengths whose epilogue fills the register arrays (`GEN_MAX_EPI`).

The check is per COLUMN, against the packed frame the kernel transforms: with a_c = frame * window and b_c = frame *
diff_window (float32 products, as the kernel forms them) the kernel transforms z_c = a_c - i b_c and separates the
two spectra by Hermitian symmetry, so the rounding of both outputs scales with ||z_c||_2:

    e_c = max_f |out[f, c] - ref[f, c]| / (eps32 ||z_c||_2)       asserted  max_c e_c <= K  for Sx and for dSx

A fault confined to one frame lane, to the partial last group of frames or to one remapped workgroup cannot hide
behind a loud column elsewhere, as it can under `relmax` of the whole transform. `K` is 4 x the largest figure of this
engine's rocFFT route (`SSQ_DEBUG_STFT_GENERIC=1`) on the same inputs over the whole table -- the yardstick that is not
the code under test; the factor is for the odd primes' butterflies, direct sums of up to 15 chained multiply-adds per
output where a radix-2/4 network has log2 of them. profiles/stft_lengths.txt holds both routes' figures per length.
"""
import collections
import contextlib
import os

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)

# 4 x 11.715, the rocFFT route's largest max_c e_c on the MI355X over LENGTHS and POW2, both shapes, Sx and dSx (n_fft =
# 1054, Sx); the fused kernels' largest there: 7.41 (n_fft = 2187, Sx), on the remapped grids 8.29
# (profiles/stft_lengths.txt)
K = 46.86

GEN_MAX_PASSES = 10
GEN_MAX_EPI = 10
GEN_NT = 256
GEN_LDS_BYTES = 78 * 1024
XCD_FROM = 64                                    # workgroups from which launch_stft_generic remaps the grid

Entry = collections.namedtuple('Entry', 'radix G why')      # radix None: the plan's route is 'rocfft'

_PRIMES = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31)
LENGTHS = {}


def _add(n, radix, G, why):
    if n in LENGTHS:
        assert LENGTHS[n][:2] == (radix, G), n
        why = LENGTHS[n].why + '; ' + why
    LENGTHS[n] = Entry(radix, G, why)


# a single pass: the first arm alone, straight into the epilogue
for _r in (2, 3, 4, 5, 7, 8, 11, 13, 16, 17, 19, 23, 29, 31):
    _add(_r, (_r,), 16, 'a single pass of radix %d' % _r)
# each odd prime first, 31 last; 961: the same radix first and last
for _n, _r, _G in ((93, 3, 16), (155, 5, 16), (217, 7, 8), (341, 11, 4), (403, 13, 4), (527, 17, 4), (589, 19, 4),
                   (713, 23, 4), (899, 29, 4), (961, 31, 4)):
    _add(_n, (_r, 31), _G, 'radix %d first, 31 last' % _r)
# each odd prime last
_add(9, (3, 3), 16, 'radix 3 last')
for _r in _PRIMES[1:]:
    _add(3 * _r, (3, _r), 16, 'radix %d last' % _r)
# each odd prime in the middle
for _n, _r, _G in ((186, 3, 8), (310, 5, 8), (434, 7, 4), (682, 11, 4), (806, 13, 4), (1054, 17, 4), (1178, 19, 4),
                   (1426, 23, 2), (1798, 29, 2), (1922, 31, 2)):
    _add(_n, (2, _r, 31), _G, 'radix %d in the middle' % _r)
# the power-of-two radices behind a first pass
_add(32, (16, 2), 16, 'radix 2 last behind 16')
_add(64, (16, 4), 16, 'radix 4 last behind 16')
_add(384, (16, 8, 3), 4, 'radix 8 in the middle')
_add(96, (16, 2, 3), 16, 'radix 2 in the middle')
_add(4096, (16, 16, 16), 1, 'radix 16 in the middle and last, G = 1')
_add(3072, (16, 16, 4, 3), 1, 'radix 4 in the middle, G = 1')
_add(20, (4, 5), 16, 'radix 4 first')
_add(40, (8, 5), 16, 'radix 8 first')
# both sides of every G edge; 1248, 2496, 4992: the epilogue's register arrays full
_add(156, (4, 3, 13), 16, 'the last length at G = 16')
_add(160, (16, 2, 5), 8, 'the first length at G = 8 that the kernel takes')
_add(312, (8, 3, 13), 8, 'the last length at G = 8')
_add(315, (3, 3, 5, 7), 4, 'the first length at G = 4 that the kernel takes')
_add(1248, (16, 2, 3, 13), 4, 'the last length at G = 4, GEN_MAX_EPI epilogue points')
_add(1250, (2, 5, 5, 5, 5), 2, 'the first length at G = 2')
_add(2496, (16, 4, 3, 13), 2, 'the last length at G = 2, GEN_MAX_EPI epilogue points')
_add(2499, (3, 7, 7, 17), 1, 'the first length at G = 1 that the kernel takes')
_add(4992, (16, 8, 3, 13), 1, 'the last length of the kernel, GEN_MAX_EPI epilogue points, the LDS full')
_add(4998, None, None, 'past the LDS: rocFFT (2 x 3 x 7 x 7 x 17, every factor a radix)')
_add(5000, None, None, 'past the LDS: rocFFT')
_add(97, None, None, 'a prime above 31: rocFFT')
_add(74, None, None, 'a prime factor above 31 (2 x 37): rocFFT')
# the lengths of the remapped grids and of the frame-position test
_add(60, (4, 3, 5), 16, 'the remapped grid at G = 16')
_add(598, (2, 13, 23), 4, "the reference's published ssq_stft shape; the remapped grid at G = 4")
# the most passes
_add(4374, (2, 3, 3, 3, 3, 3, 3, 3), 1, 'eight passes')
_add(2187, (3, 3, 3, 3, 3, 3, 3), 2, 'seven passes of one radix')

FULL_EPILOGUE = (1248, 2496, 4992)
G_EDGES = ((156, 160), (312, 315), (1248, 1250), (2496, 2499), (4992, 4998))
# stft_fused_kernel: frames per workgroup (4096 points / n_fft)
POW2 = {128: 32, 256: 16, 512: 8, 1024: 4, 2048: 2}
# the lengths that are cheap under the emulator (a work-item is a host thread there)
EMULATED = tuple(n for n, e in LENGTHS.items() if e.radix and len(e.radix) == 1) + (
    156, 160, 312, 315, 1248, 1250, 2496, 2499, 4992, 4998, 961, 1798, 4374)


def plan_rule(n):
    """(radix tuple, G) of `stft_generic_plan` restated from its header comment, or None where it refuses: the
    factors in the order 16s, 8s, 4s, 2s, then 3 .. 31 ascending; at most 10 of them; two buffers of n x G x 8 bytes
    within 78 KB -- G = 16 halved down to 4 while they pass 39 KB (four workgroups per CU), then down to 1 while they
    pass 78 KB."""
    if n < 2:
        return None
    radix, m = [], n
    for r in (16, 8, 4, 2) + _PRIMES:
        while m % r == 0:
            radix.append(r)
            m //= r
    if m != 1 or len(radix) > GEN_MAX_PASSES or 16 * n > GEN_LDS_BYTES:
        return None
    G = 16
    while G > 4 and 16 * n * G > GEN_LDS_BYTES // 2:
        G //= 2
    while G > 1 and 16 * n * G > GEN_LDS_BYTES:
        G //= 2
    return tuple(radix), G


def expected_algo(n):
    """The route of a float32 plan of window length `n` (`ssq_stft_plan_create`)."""
    if n in POW2:
        return 'fused'
    return 'fused-mixed-radix' if plan_rule(n) else 'rocfft'


def query(lib, n):
    """`ssq_stft_generic_shape`: (radix tuple, G), or None where the mixed-radix kernel does not take `n`."""
    import ctypes
    radix, npass, G = (ctypes.c_int * GEN_MAX_PASSES)(), ctypes.c_int(-1), ctypes.c_int(-1)
    took = lib.ssq_stft_generic_shape(int(n), radix, ctypes.byref(npass), ctypes.byref(G))
    assert took in (0, 1)
    if not took:
        assert npass.value == 0 and G.value == 0 and not any(radix)
        return None
    assert 1 <= npass.value <= GEN_MAX_PASSES and not any(radix[npass.value:])
    return tuple(radix[:npass.value]), G.value


def epilogue_points(n, G):
    """epilogue points a work-item of the mixed-radix kernel holds: ceil((n / 2 + 1) G / 256)"""
    return -(-(n // 2 + 1) * G // GEN_NT)


def shapes(n_fft, G):
    """The two shapes a length runs at. Modulated: hop n_fft // 3, 3 G + 1 frames (5 for G = 1): the last workgroup
    holds one frame. Not modulated: hop 1, zero padding, 2 G + 3 frames."""
    G = G or 1
    hop = max(1, n_fft // 3)
    n_hops = 3 * G + 1 if G > 1 else 5
    return (dict(hop=hop, N=(n_hops - 1) * hop + 1, n_hops=n_hops, modulated=True, padtype='reflect'),
            dict(hop=1, N=2 * G + 3, n_hops=2 * G + 3, modulated=False, padtype='zero'))


def signal(N, seed, B=0):
    """two_chirps in float32 (what the device is handed), `B` of them stacked when B > 0"""
    from conftest import two_chirps
    x = np.stack([two_chirps(N, seed=seed + 17 * b) for b in range(max(B, 1))]).astype(np.float32)
    return x if B else x[0]


# ---- the float64 statement ---------------------------------------------------------------------------------------
def window_spec(n_fft):
    """The `window` argument: the default (DPSS) where its design accepts the length (time-bandwidth product
    max(4, n // 8) needs n > 8), a Hamming window for the very short ones."""
    return None if n_fft >= 16 else 'hamming'


def windows(S, n_fft, modulated, fs=1.):
    """(window, diff_window) as the plan is handed them: rotated with the frame when modulated, float32."""
    win, dwin = S.get_window(window_spec(n_fft), n_fft, n_fft, derivative=True, dtype='float32')
    if modulated:
        win, dwin = np.fft.ifftshift(win), np.fft.ifftshift(dwin) * fs
    return win.astype(np.float32), dwin.astype(np.float32)


def pad_sources(S, N, n_fft, padtype):
    """Source sample of every padded position (-1: a zero), read off the padding of 1..N: the rule of
    `ssq_stft_plan_create` -- padded length N + n_fft - 1, the odd sample on the left."""
    xp = S.padsignal(np.arange(1, N + 1.), padtype, padlength=N + n_fft - 1)
    return np.rint(xp).astype(np.int64) - 1


def pad_sources_numpy(N, n_fft, padtype):
    """The same table from np.pad (test_stft_lengths_design.py holds the two together)."""
    tot = n_fft - 1
    n2 = tot // 2
    mode = {'zero': 'constant', 'reflect': 'reflect', 'symmetric': 'symmetric', 'replicate': 'edge', 'wrap': 'wrap'}
    return np.pad(np.arange(N), (tot - n2, n2), mode=mode[padtype], **(
        dict(constant_values=-1) if padtype == 'zero' else {}))


def statement(x, win, dwin, n_fft, hop, src, modulated):
    """`stft` with its derivative in float64 on float32 data `x` (N,): Sx, dSx (n_fft // 2 + 1, n_hops) and the norms
    ||z_c||_2 of the packed frames. Frame j starts at padded sample j hop; modulated: rotated left by n_fft // 2 (which
    is right by ceil(n_fft / 2): utils/stft_utils.py:76-82); the products frame * window, frame * diff_window
    rounded to float32 as the kernel forms them, then np.fft.rfft."""
    assert x.dtype == np.float32 and win.dtype == np.float32 and dwin.dtype == np.float32
    xp = np.where(src >= 0, x[np.clip(src, 0, None)], np.float32(0))
    n_hops = (len(xp) - n_fft) // hop + 1
    fr = xp[np.arange(n_hops)[:, None] * hop + np.arange(n_fft)[None, :]]
    if modulated:
        fr = np.roll(fr, -(n_fft // 2), axis=1)
    a, b = fr * win[None, :], fr * dwin[None, :]
    assert a.dtype == np.float32 and b.dtype == np.float32
    a, b = a.astype(np.float64), b.astype(np.float64)
    return dict(Sx=np.fft.rfft(a, axis=1).T, dSx=np.fft.rfft(b, axis=1).T,
                znorm=np.sqrt((a * a + b * b).sum(axis=1)))


def column_errors(out, ref, znorm):
    """e_c of the module's docstring, per column (a silent column must be exactly zero: inf otherwise)."""
    d = np.abs(out.astype(np.complex128) - ref).max(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.where(znorm > 0, d / (EPS32 * znorm), np.where(d > 0, np.inf, 0.))
    return np.where(np.isnan(e), np.inf, e)          # (a point nobody wrote: `poisoned_outputs`)


# ---- one run of the device (or the emulated) transform -----------------------------------------------------------
@contextlib.contextmanager
def poisoned_outputs():
    """`torch.empty` hands out NaNs for the duration: the plan allocates its outputs with it, and the allocator likes to
    hand back the block that held the previous call's -- correct -- result, so a column no workgroup wrote (a
    remapped block that went to the wrong place) would otherwise pass."""
    import torch
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point() or t.is_complex():
            t.fill_(float('nan'))
        return t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def run_stft(S, x, n_fft, hop, modulated, padtype, rocfft=False):
    """`S.stft` with its derivative on float32 `x` ((N,) or (B, N)) through a fresh plan, `rocfft`: this engine's
    rocFFT route (`SSQ_DEBUG_STFT_GENERIC=1`, read when a plan is made). Returns Sx, dSx and the plan's route."""
    from ssqueezepy_amd import _stft
    saved = os.environ.pop('SSQ_DEBUG_STFT_GENERIC', None)
    if rocfft:
        os.environ['SSQ_DEBUG_STFT_GENERIC'] = '1'
    _stft._PLAN_CACHE.clear()
    try:
        with poisoned_outputs():
            Sx, dSx = S.stft(x, window=window_spec(n_fft), n_fft=n_fft, hop_len=hop, modulated=modulated,
                             padtype=padtype, derivative=True, dtype='float32', astensor=False)
        algo = list(_stft._PLAN_CACHE.values())[-1].algo
    finally:
        os.environ.pop('SSQ_DEBUG_STFT_GENERIC', None)
        if saved is not None:
            os.environ['SSQ_DEBUG_STFT_GENERIC'] = saved
        _stft._PLAN_CACHE.clear()
    return Sx, dSx, algo


def figures(S, x, n_fft, hop, modulated, padtype, rocfft=False):
    """max_c e_c of Sx and of dSx (over every signal of a batch) for one run, the column and signal of each, and
    the route."""
    Sx, dSx, algo = run_stft(S, x, n_fft, hop, modulated, padtype, rocfft)
    xs = x if x.ndim == 2 else x[None]
    Sx, dSx = (v if x.ndim == 2 else v[None] for v in (Sx, dSx))
    win, dwin = windows(S, n_fft, modulated)
    src = pad_sources(S, xs.shape[-1], n_fft, padtype)
    out = dict(algo=algo, Sx=0., dSx=0., at={})
    for b in range(len(xs)):
        ref = statement(xs[b], win, dwin, n_fft, hop, src, modulated)
        assert Sx[b].shape == ref['Sx'].shape, (Sx[b].shape, ref['Sx'].shape)
        for k, v in (('Sx', Sx[b]), ('dSx', dSx[b])):
            e = column_errors(v, ref[k], ref['znorm'])
            if e.max() >= out[k]:
                out[k], out['at'][k] = float(e.max()), (b, int(e.argmax()))
    return out


def check_columns(S, x, n_fft, hop, modulated, padtype, algo, what):
    """The per-column bound on one run; returns the figures."""
    f = figures(S, x, n_fft, hop, modulated, padtype)
    assert f['algo'] == algo, (what, f['algo'])
    assert f['Sx'] <= K and f['dSx'] <= K, (what, f)
    return f
