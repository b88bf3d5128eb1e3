# -*- coding: utf-8 -*-
"""`conceft_stft`, `algos.conceft_gpu` and the entry `ssq_conceft` (ConceFT: multitaper synchrosqueezing in one
kernel).

The oracle of the kernel is `conceft.statement`: the entry's definition in NumPy on separate real float64
arrays, one ufunc per operation, in the stated order. The kernel evaluates the same operations in float64, so on
every column without a point within 1e-6 (relative) of `gamma` -- where the device's `hypot` and libm's may
disagree on the branch -- the bins and the order of every sum are the statement's, and what may differ is `hypot`
itself, an ulp per term of the average over the projections: `conceft.check` holds the bounds.
Two links to entries that exist independently of the statement pin the plane and projection indexing: unit
projections against `phase_stft_gpu` + `indexed_sum_onfly` per plane.
"""
import ctypes
import os
import numpy as np
import pytest
from conftest import report_measured
import conceft
from conceft import _np, FS, EPS64

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
# end to end
N, N_FFT, J3, Q6 = 2048, 128, 3, 6


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


_CASES = {}


def case(shape, dtype):
    """Planes, projections, `Sfs`, a `gamma` midway between two neighbouring samples of ``|Vq|`` at the median (the
    skip branch takes half the points) and the columns to leave out; made once, nobody writes to them."""
    key = (shape, dtype)
    if key not in _CASES:
        V, dV, proj, Sfs = conceft.planes(shape, dtype)
        mags = conceft.magnitudes(V, proj)
        gamma = conceft.above_median(mags)
        assert .45 <= (mags < gamma).mean() <= .55
        _CASES[key] = (V, dV, proj, Sfs, gamma, conceft.near_gamma_columns(mags, gamma))
    return _CASES[key]


_REFS = {}


def reference(shape, dtype, flipud, average):
    key = (shape, dtype, flipud, average)
    if key not in _REFS:
        V, dV, proj, Sfs, gamma, _ = case(shape, dtype)
        _REFS[key] = conceft.statement(V, dV, Sfs, proj, gamma, Sfs, flipud, average)
    return _REFS[key]


def run(S, V, dV, Sfs, proj, gamma, flipud=False, average='abs', ssq_freqs=None):
    return S.conceft_gpu(list(V), list(dV), Sfs, proj, Sfs if ssq_freqs is None else ssq_freqs, gamma, flipud, average)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('average', ['abs', 'complex'])
@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', conceft.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_vs_statement(S, shape, dtype, flipud, average):
    V, dV, proj, Sfs, gamma, near = case(shape, dtype)
    ref = reference(shape, dtype, flipud, average)
    # the grid spans Sfs: interior bins, bin 0 and the top bin all receive points
    filled = (ref != 0).any(axis=(0, 2))
    assert filled[0] and filled[-1] and filled[1:-1].any()
    Cx = run(S, V, dV, Sfs, proj, gamma, flipud, average)
    conceft.check('conceft_kernel_%s_%s_%d_%s' % ('x'.join(map(str, shape)), dtype, flipud, average), Cx, ref, near,
                  shape[2], dtype, average)


def _two_step(S, Vj, dVj, Sfs, gamma, flipud):
    return S.indexed_sum_onfly(Vj, S.phase_stft_gpu(Vj, dVj, Sfs, gamma), Sfs, 1, False, flipud)


@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
def test_unit_projections_are_the_two_step_path_per_plane(S, flipud):
    """``proj = I_J``: `Cx` is the mean over the planes of ``|indexed_sum_onfly(V_j, phase_stft_gpu(V_j, dV_j))|``."""
    import torch
    shape = (2, 3, 3, 33, 50)
    V, dV, _, Sfs = conceft.planes(shape, 'float64')
    gamma = conceft.above_median(np.abs(V))
    Vd, dVd = [dev(p) for p in V], [dev(p) for p in dV]
    Cx = _np(run(S, Vd, dVd, Sfs, np.eye(3), gamma, flipud))
    parts = [_np(torch.abs(_two_step(S, Vd[j], dVd[j], Sfs, gamma, flipud))) for j in range(3)]
    ref = (parts[0] + parts[1] + parts[2]) / 3.
    err = np.abs(Cx - ref)
    bound = (4 + 3) * EPS64 * np.abs(ref)
    report_measured('conceft_unit_projections_%d' % flipud,
                    max_err_over_bound=float((err[bound > 0] / bound[bound > 0]).max()))
    assert (ref != 0).mean() > .1 and (err <= bound).all()


def test_one_plane_one_projection_complex_is_indexed_sum(S):
    V, dV, _, Sfs = conceft.planes((2, 1, 1, 33, 50), 'float64')
    gamma = conceft.above_median(np.abs(V))
    Vd, dVd = dev(V[0]), dev(dV[0])
    Cx = run(S, [Vd], [dVd], Sfs, np.ones((1, 1)), gamma, average='complex')
    assert np.array_equal(_np(Cx), _np(_two_step(S, Vd, dVd, Sfs, gamma, False)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    import torch
    shape = (3, 2, 3, 33, 50)
    V, dV, proj, Sfs, gamma, _ = case(shape, dtype)
    Vd, dVd = [dev(p) for p in V], [dev(p) for p in dV]
    for average in ('abs', 'complex'):
        Cx = run(S, Vd, dVd, Sfs, proj, gamma, average=average)
        assert torch.equal(Cx, run(S, Vd, dVd, Sfs, proj, gamma, average=average))
        for b in range(3):
            one = run(S, [p[b] for p in Vd], [p[b] for p in dVd], Sfs, proj, gamma, average=average)
            assert one.shape == Cx.shape[1:] and torch.equal(Cx[b], one), (average, b)


@pytest.mark.parametrize('dtype', DTYPES)
def test_column_below_gamma_gives_zeros(S, dtype):
    shape = (1, 2, 3, 33, 50)
    V, dV, proj, Sfs, gamma, _ = case(shape, dtype)
    V = V.copy()
    V[..., 17] *= 1e-6                        # |Vq| <= sum_j |V_j| < gamma on the whole column
    assert conceft.magnitudes(V, proj)[..., 17].max() < .5 * gamma
    Cx = _np(run(S, V, dV, Sfs, proj, gamma))
    assert (Cx[..., 17] == 0).all() and (Cx[..., 16] != 0).any() and (Cx[..., 18] != 0).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """Planes handed over as views -- a column slice (strided, offset pointer), a lazy conjugate, every second row, a
    wider dtype -- give the bits of the plain planes (tests/test_gpu_input_layouts.py)."""
    import torch
    shape = (2, 2, 3, 33, 50)
    V, dV, proj, Sfs, gamma, _ = case(shape, dtype)
    B, J, Q, rows, n = shape
    want = run(S, [dev(p) for p in V], [dev(p) for p in dV], Sfs, proj, gamma)
    big = torch.zeros((B, rows, n + 3), dtype=dev(V[0]).dtype, device=DEV)
    big[..., 1:-2] = dev(V[0])
    col_slice = big[..., 1:-2]
    assert not col_slice.is_contiguous() and col_slice.data_ptr() != big.data_ptr()
    conj = dev(np.conj(V[1])).conj()
    assert conj.is_conj()
    tall = torch.zeros((B, 2 * rows, n), dtype=conj.dtype, device=DEV)
    tall[:, ::2] = dev(dV[0])
    wider = dev(dV[1].astype(np.complex128 if dtype == 'float32' else np.complex64))
    got = run(S, [col_slice, conj], [tall[:, ::2], wider if dtype == 'float32' else dev(dV[1])], Sfs, proj, gamma)
    assert torch.equal(got, want)
    assert torch.equal(run(S, V, dV, Sfs, proj, gamma), want)              # NumPy planes


def test_abi_refusals_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    lib = _lib.load()
    assert lib.ssq_version() >= 111 and 'ssq_conceft' in _lib.EXPORTS
    B, J, Q, rows, n = 1, 2, 3, 9, 11
    V, dV, proj, Sfs = conceft.planes((B, J, Q, rows, n), 'float64')
    Vd, dVd, sfs = [dev(p) for p in V], [dev(p) for p in dV], dev(Sfs)
    kind, p = ssq_grid_params(Sfs, False)
    good = dict(V=[t.data_ptr() for t in Vd], dV=[t.data_ptr() for t in dVd], Sfs=sfs.data_ptr(),
                proj=np.ascontiguousarray(np.stack([proj.real, proj.imag], -1)), batch=B, J=J, Q=Q, rows=rows, n=n,
                gamma=.5)
    Cx = torch.full((B, rows, n), -7., dtype=torch.float64, device=DEV)

    def call(**kw):
        a = dict(good, **kw)
        ptrs = ctypes.c_void_p * 8
        r = np.ascontiguousarray(a['proj'], dtype=np.float64)
        return lib.ssq_conceft(_lib.F64, ptrs(*a['V']), ptrs(*a['dV']), a['Sfs'], r.ctypes.data, Cx.data_ptr(),
                               a['batch'], a['J'], a['Q'], a['rows'], a['n'], a['gamma'], kind, _lib.params5(p), 0, 0, None)
    bad_proj = good['proj'].copy()
    bad_proj[1, 1, 0] = np.inf
    nan_proj = good['proj'].copy()
    nan_proj[2, 0, 1] = np.nan
    refused = [dict(J=0), dict(J=9), dict(Q=0), dict(Q=1025, proj=np.zeros((1025, J, 2))), dict(rows=1), dict(batch=0),
               dict(n=0), dict(batch=1 << 20, rows=64, n=64), dict(V=[Vd[0].data_ptr(), None]),
               dict(dV=[None, dVd[1].data_ptr()]), dict(proj=bad_proj), dict(proj=nan_proj), dict(gamma=-1.),
               dict(gamma=float('nan')), dict(rows=1281)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_conceft'), (kw, lib.ssq_last_error())
        assert bool((Cx == -7.).all()), kw
    assert call() == 0
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((Cx == -7.).any())


# ------------------------------------------------------------------------------------------ end to end
def tones(bins, N=N, n_fft=N_FFT):
    t = np.arange(N)
    return sum(np.cos(2 * np.pi * b / n_fft * t + .3 * k) for k, b in enumerate(bins))


def own_planes(S, x, J, dtype):
    """The `J` STFTs and derivative planes `conceft_stft` hands to the kernel, from the package's own plans."""
    import torch
    from ssqueezepy_amd import _stft
    H, dH = S.hermite_windows(J, N_FFT, N_FFT, 6., dtype)
    xd = torch.as_tensor(np.asarray(x).astype(dtype)).to(DEV)
    B = 1 if x.ndim == 1 else x.shape[0]
    outs = [_stft.get_stft_plan(x.shape[-1], N_FFT, 1, H[j], dH[j], 1., 'reflect', True, dtype, B)
            .execute(xd, want_dSx=True) for j in range(J)]
    return [o['Sx'] for o in outs], [o['dSx'] for o in outs]


@pytest.mark.parametrize('average', ['abs', 'complex'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_conceft_stft_vs_statement_on_its_own_planes(S, dtype, average, N=N):
    import torch
    from ssqueezepy_amd._conceft import draw_projections
    x = tones([16, 40], N) + .1 * np.random.default_rng(3).standard_normal(N)
    Cx, Sxs, ssq_freqs, Sfs = S.conceft_stft(x, J3, Q6, n_fft=N_FFT, fs=1., seed=5, dtype=dtype, average=average)
    assert Cx.shape == (N_FFT // 2 + 1, N) and len(Sxs) == J3 and not Cx.requires_grad
    assert np.array_equal(Sfs, np.linspace(0, .5, N_FFT // 2 + 1, dtype=dtype)) and np.array_equal(ssq_freqs, Sfs)
    Vs, dVs = own_planes(S, x, J3, dtype)
    for a, b in zip(Sxs, Vs):
        assert torch.equal(a, b)
    V, dV = [np.stack([_np(p)[None] for p in P]) for P in (Vs, dVs)]
    proj = conceft.unit_rows(draw_projections(Q6, J3, 5))
    gamma = 10 * float(np.finfo(dtype).eps)
    near = conceft.near_gamma_columns(conceft.magnitudes(V, proj), gamma)
    ref = conceft.statement(V, dV, Sfs, proj, gamma, Sfs, False, average)
    conceft.check('conceft_stft_%s_%s' % (dtype, average), _np(Cx)[None], ref, near, Q6, dtype, average)


def test_seed_and_explicit_projections_give_the_same_bits(S, N=N):
    import torch
    from ssqueezepy_amd._conceft import draw_projections
    x = np.stack([tones([16, 40], N), tones([25], N)])
    kw = dict(n_tapers=J3, n_proj=Q6, n_fft=N_FFT, fs=1.)
    a = S.conceft_stft(x, seed=11, **kw)[0]
    assert a.shape == (2, N_FFT // 2 + 1, N)
    assert torch.equal(a, S.conceft_stft(x, seed=11, **kw)[0])
    assert torch.equal(a, S.conceft_stft(x, proj=draw_projections(Q6, J3, 11), **kw)[0])
    assert not torch.equal(a, S.conceft_stft(x, seed=12, **kw)[0])
    flipped, _, freqs, Sfs = S.conceft_stft(x, seed=11, flipud=True, **kw)
    assert torch.equal(flipped, a.flip(-2)) and np.array_equal(freqs, Sfs[::-1])
    with pytest.raises(ValueError, match='linearly distributed'):
        S.conceft_stft(x[0], ssq_freqs=np.geomspace(.01, .5, N_FFT // 2 + 1), **kw)


def row_energy(C):
    return (np.abs(_np(C)).astype(np.float64) ** 2).sum(axis=-1)


def test_two_tones_land_on_their_rows(S, N=N):
    Cx = S.conceft_stft(tones([16, 40], N), J3, Q6, n_fft=N_FFT, fs=1.)[0]
    e = row_energy(Cx)
    e[:3] = e[-3:] = 0
    assert sorted(np.argsort(e)[-2:]) == [16, 40]


def test_noisy_tone_is_no_less_concentrated_than_ssq_stft(S):
    """A tone in white noise at 0 dB: the share of the energy within +-2 rows of the tone, ConceFT (J = 3, Q = 30)
    against ``abs(ssq_stft)`` on the same call. Asserted: ConceFT's share is not the lower one. The shares
    themselves are recorded (profiles/conceft.txt)."""
    rng = np.random.default_rng(2016)
    row = 20
    x = tones([row]) + np.sqrt(.5) * rng.standard_normal(N)
    kw = dict(n_fft=N_FFT, fs=1.)
    Cx = S.conceft_stft(x, 3, 30, **kw)[0]
    Tx = S.ssq_stft(x, **kw)[0]
    shares = [float(e[row - 2:row + 3].sum() / e.sum()) for e in (row_energy(Cx), row_energy(Tx))]
    report_measured('conceft_noisy_tone_share', conceft=shares[0], ssq_stft=shares[1])
    assert shares[0] >= shares[1], shares
