# -*- coding: utf-8 -*-
"""The fixture of the parent commit's bits for the host FFT layer (csrc/ssq_fft.h: the rocFFT plan wrapper, the
per-stream plan caches): one call through every rocFFT user, on seeded inputs, on the MI355X.

    python tests/host_fft.py [--out FILE]

records tests/golden/host_fft_parent.npz with the library in place (`SSQ_HIP_LIB` selects another build): run it at
the parent commit of a change to that layer, commit the file, and
tests/test_gpu_inverse.py::test_host_fft_parent_bits holds the change to it. The bits are rocFFT's on gfx950: there is
no emulated twin."""
import os
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'host_fft_parent.npz')
# (dtype, n_fft, hop, N): float64 takes the rocFFT routes at any n_fft; 74 = 2 * 37 has a prime factor above 31,
# which no fused float32 kernel takes
STFT_CASES = [('float64', 64, 16, 300), ('float32', 74, 14, 300)]
ROWS, COLS = 8, 128             # icwt(one_int=False), trigdiff
CWT_N = 150                     # cwt without padding: a transform length that is no power of two


def _cdt(dtype):
    return np.complex64 if dtype == 'float32' else np.complex128


def _complex(rng, shape, dtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(_cdt(dtype))


def make_inputs():
    rng = np.random.default_rng(2026)
    z = {}
    for dtype, n_fft, hop, N in STFT_CASES:
        z['in_x_' + dtype] = rng.standard_normal(N).astype(dtype)
        z['in_gSx_' + dtype] = _complex(rng, (n_fft // 2 + 1, (N - 1) // hop + 1), dtype)
        z['in_gx_' + dtype] = rng.standard_normal(N).astype(dtype)
        z['in_W_' + dtype] = _complex(rng, (ROWS, COLS), dtype)
    z['in_cwt_x'] = rng.standard_normal(CWT_N)
    return z


def run_calls(S, z, dev):
    """name -> result (NumPy) of every call, on the inputs `z` (the `in_*` arrays of the fixture)."""
    import torch

    def t(a):
        return torch.as_tensor(a, device=dev)

    out = {}
    for dtype, n_fft, hop, N in STFT_CASES:
        kw = dict(n_fft=n_fft, hop_len=hop)
        x = t(z['in_x_' + dtype]).requires_grad_(True)
        Sx = S.stft(x, dtype=dtype, **kw)
        out['stft_' + dtype] = Sx
        out['stft_backward_' + dtype] = torch.autograd.grad(Sx, x, t(z['in_gSx_' + dtype]))[0]
        Sd = Sx.detach().clone().requires_grad_(True)
        assert S.algos.istft_algo(dtype, n_fft, Sd.shape[-1], hop, N) == 'rocfft'
        xr = S.istft(Sd, N=N, **kw)
        out['istft_' + dtype] = xr
        out['istft_backward_' + dtype] = torch.autograd.grad(xr, Sd, t(z['in_gx_' + dtype]))[0]
        W = t(z['in_W_' + dtype])
        wav = S.Wavelet(('gmw', {'dtype': dtype}))
        out['icwt2_' + dtype] = S.icwt(W, wav, scales=2. ** (1 + np.arange(ROWS) / 4.), nv=4, one_int=False)
        out['trigdiff_' + dtype] = S.trigdiff(W, fs=1., padtype='reflect', N=COLS)
    wav = S.Wavelet(('gmw', {'dtype': 'float64'}))
    out['cwt_float64'] = S.cwt(t(z['in_cwt_x']), wav, scales='log', nv=4, padtype=None)[0]
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def record_parent(S, out, dev='cuda'):
    z = make_inputs()
    res = run_calls(S, z, dev)
    for k, v in res.items():
        assert np.isfinite(v.view(v.real.dtype)).all() and np.abs(v).max() > 0, k
        z['out_' + k] = v
    np.savez(out, **z)
    return out


def assert_parent_bits(S, dev='cuda'):
    """Every call's result on the fixture's inputs has the bits the parent commit's library gave."""
    with np.load(GOLDEN) as f:
        z = {k: f[k] for k in f.files}
    res = run_calls(S, z, dev)
    assert sorted('out_' + k for k in res) == sorted(k for k in z if k.startswith('out_'))
    differ = {}
    for k, v in res.items():
        ref = z['out_' + k]
        assert v.shape == ref.shape and v.dtype == ref.dtype, k
        n = int((v.view(np.uint8) != ref.view(np.uint8)).reshape(-1, v.dtype.itemsize).any(axis=1).sum())
        if n:
            differ[k] = n
    assert not differ, differ


if __name__ == '__main__':
    import argparse
    import sys
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ssqueezepy_amd
    print(record_parent(ssqueezepy_amd, a.out))
