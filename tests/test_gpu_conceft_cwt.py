# -*- coding: utf-8 -*-
"""`conceft_cwt`, `algos.conceft_cwt_gpu` and the entry `ssq_conceft_cwt` (ConceFT for the CWT: multitaper
synchrosqueezing over Morse wavelets of increasing order, in one kernel).

The oracle of the kernel is `conceft_cwt.projections` / `average_of`: the entry's definition in NumPy on separate real
float64 arrays, one ufunc per operation, in the stated order. The kernel evaluates the same operations in float64, so
on every column without a point within 1e-6 (relative) of `gamma` or within 1e-9 of a bin's rounding boundary -- where
the device's `hypot` / `log2` and libm's may disagree on a branch -- the bins and the order of every sum are the
statement's, and what may differ is `hypot` itself, an ulp per term of the average over the projections:
`conceft_cwt.check_cwt` holds the bounds. A link to entries that exist independently of the statement pins the
indexing and the weight: one plane, one unit projection against `phase_cwt_gpu` + `indexed_sum_onfly`.
"""
import ctypes
import os
import numpy as np
import pytest
from conftest import report_measured
import conceft
import conceft_cwt as cc
from conceft import _np, EPS64

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
# end to end
N, NV, J3, Q5 = 2048, 16, 3, 5


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


_CASES = {}


def case(shape, dtype):
    """Planes, projections, weights, a `gamma` midway between two neighbouring samples of ``|Wq|`` at the median (the
    skip branch takes half the points) and the columns with a point near `gamma`; made once, nobody writes to them."""
    key = (shape, dtype)
    if key not in _CASES:
        W, dW, proj, cst = cc.planes(shape, dtype)
        mags = conceft.magnitudes(W, proj)
        gamma = conceft.above_median(mags)
        assert .4 <= (mags < gamma).mean() <= .6
        _CASES[key] = (W, dW, proj, cst, gamma, conceft.near_gamma_columns(mags, gamma))
    return _CASES[key]


_PROJS = {}


def projections(shape, dtype, grid):
    """The statement's `Tq` of a case on a grid, and the columns to leave out (near `gamma` or near a boundary)."""
    key = (shape, dtype, grid)
    if key not in _PROJS:
        W, dW, proj, cst, gamma, near = case(shape, dtype)
        Tr, Ti, nb = cc.projections(W, dW, cst, proj, gamma, cc.ssq_freqs(grid, shape[3]))
        _PROJS[key] = (Tr, Ti, near | nb)
    return _PROJS[key]


def run(S, W, dW, cst, proj, gamma, freqs, flipud=False, average='abs', out=None):
    return S.conceft_cwt_gpu(list(W), list(dW), proj, freqs, cst, gamma, flipud, average, out)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def shape_id(s):
    return 'x'.join(map(str, s))


@pytest.mark.parametrize('average', ['abs', 'complex'])
@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', cc.GRIDS)
@pytest.mark.parametrize('shape', cc.SHAPES, ids=shape_id)
def test_kernel_vs_statement(S, shape, grid, dtype, flipud, average):
    W, dW, proj, cst, gamma, _ = case(shape, dtype)
    Tr, Ti, near = projections(shape, dtype, grid)
    ref = cc.average_of(Tr, Ti, flipud, average)
    # `w` leaves the grid at both ends: bin 0, the top bin and interior bins all receive points
    filled = (ref != 0).any(axis=(0, 2))
    assert filled[0] and filled[-1] and filled[1:-1].any()
    Cx = run(S, W, dW, cst, proj, gamma, cc.ssq_freqs(grid, shape[3]), flipud, average)
    cc.check_cwt('conceft_cwt_kernel_%s_%s_%s_%d_%s' % (shape_id(shape), grid, dtype, flipud, average), Cx, ref, near,
                 shape[2], dtype, average)


@pytest.mark.parametrize('grid', cc.GRIDS)
def test_a_rows_weight_shows_where_its_terms_land(S, grid):
    """`cst` of ones against `cst` with row 11 doubled: `Cx` differs exactly in the cells that row's terms reach."""
    shape = (2, 2, 1, 33, 50)
    W, dW, proj, _, gamma, near = case(shape, 'float64')
    freqs = cc.ssq_freqs(grid, shape[3])
    ones, doubled = np.ones(33), np.ones(33)
    doubled[11] = 2.
    a = _np(run(S, W, dW, ones, proj, gamma, freqs, average='complex'))
    b = _np(run(S, W, dW, doubled, proj, gamma, freqs, average='complex'))
    assert np.array_equal(a, _np(run(S, W, dW, 1., proj, gamma, freqs, average='complex')))      # a scalar `const`
    only11 = np.zeros(33)
    only11[11] = 1.
    Tr, Ti, nb = cc.projections(W, dW, only11, proj, gamma, freqs)
    lands = (Tr[0] != 0) | (Ti[0] != 0)
    keep = np.broadcast_to(~(near | nb)[:, None, :], lands.shape)
    assert keep.mean() >= .99 and lands.sum() > 20 and np.array_equal((a != b)[keep], lands[keep])


@pytest.mark.parametrize('flipud', [False, True], ids=['noflip', 'flipud'])
@pytest.mark.parametrize('grid', cc.GRIDS)
def test_one_plane_one_projection_complex_is_the_two_step_path(S, grid, flipud):
    """``J = 1, Q = 1, proj = [[1]]``, 'complex', float64: `Cx` against ``indexed_sum_onfly(W, phase_cwt_gpu(W, dW,
    gamma), ssq_freqs, const, logscale, flipud)``, within ``(5 + Q) eps`` of the statement's magnitude per cell. No
    column is left out of that comparison: both sides take `hypot` and `log2` from the device. Which of the two
    differs from the statement is counted, on the columns the statement keeps, and reported. Measured on the MI355X
    and under the emulator: neither -- both form every term as ``W * cst[i]`` and add a cell's terms in ascending row
    order, so both equal the statement, and each other, bit for bit on all six cases (error over bound 0)."""
    shape = (2, 1, 1, 33, 50)
    W, dW, _, cst, _, _ = case(shape, 'float64')
    gamma = conceft.above_median(np.abs(W))
    freqs = cc.ssq_freqs(grid, shape[3])
    Wd, dWd = dev(W[0]), dev(dW[0])
    Cx = _np(run(S, [Wd], [dWd], cst, np.ones((1, 1)), gamma, freqs, flipud, 'complex'))
    two = _np(S.indexed_sum_onfly(Wd, S.phase_cwt_gpu(Wd, dWd, gamma), freqs, cst, grid != 'linear', flipud))
    Tr, Ti, nb = cc.projections(W, dW, cst, np.ones((1, 1)), gamma, freqs)
    ref = cc.average_of(Tr, Ti, flipud, 'complex')
    keep = np.broadcast_to(~nb[:, None, :], ref.shape)
    bound = (5 + 1) * EPS64 * np.abs(ref)
    err = np.abs(Cx - two)
    report_measured('conceft_cwt_two_step_link_%s_%d' % (grid, flipud),
                    max_err_over_bound=float((err[bound > 0] / bound[bound > 0]).max()),
                    fused_differs_from_statement=int((Cx != ref)[keep].sum()),
                    two_step_differs_from_statement=int((two != ref)[keep].sum()))
    assert (ref != 0).mean() > .1 and (err[keep] <= bound[keep]).all()
    assert np.array_equal((Cx == 0)[keep], (two == 0)[keep])


def test_zero_derivative_lands_in_bin_0(S):
    """``dW = 0``: ``w = 0``, whose ``log2`` is ``-inf`` -- bin 0 on every grid (the top row with `flipud`)."""
    shape = (1, 2, 3, 33, 50)
    W, dW, proj, cst, gamma, _ = case(shape, 'float64')
    for grid in cc.GRIDS:
        Cx = _np(run(S, W, np.zeros_like(dW), cst, proj, gamma, cc.ssq_freqs(grid, 33), True))
        assert (Cx[:, :-1] == 0).all() and (Cx[:, -1] != 0).all(), grid


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_repeats_and_out(S, dtype):
    import torch
    shape = (3, 2, 3, 33, 50)
    W, dW, proj, cst, gamma, _ = case(shape, dtype)
    Wd, dWd = [dev(p) for p in W], [dev(p) for p in dW]
    freqs = cc.ssq_freqs('log-piecewise', 33)
    for average in ('abs', 'complex'):
        Cx = run(S, Wd, dWd, cst, proj, gamma, freqs, average=average)
        assert torch.equal(Cx, run(S, Wd, dWd, cst, proj, gamma, freqs, average=average))
        for b in range(3):
            one = run(S, [p[b] for p in Wd], [p[b] for p in dWd], cst, proj, gamma, freqs, average=average)
            assert one.shape == Cx.shape[1:] and torch.equal(Cx[b], one), (average, b)
        out = torch.full_like(Cx, -7.)
        assert run(S, Wd, dWd, cst, proj, gamma, freqs, average=average, out=out) is out and torch.equal(out, Cx)
    with pytest.raises(ValueError, match='`out` must be'):
        run(S, Wd, dWd, cst, proj, gamma, freqs, out=torch.empty((3, 33, 51), dtype=Cx.real.dtype, device=DEV))
    with pytest.raises(ValueError, match='`const` must be'):
        run(S, Wd, dWd, cst[:-1], proj, gamma, freqs)


@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """Planes handed over as views -- a column slice (strided, offset pointer), a lazy conjugate, every second row, a
    wider dtype -- give the bits of the plain planes (tests/test_gpu_input_layouts.py); so do NumPy planes and a
    `const` handed over as a tensor."""
    import torch
    shape = (2, 2, 3, 33, 50)
    W, dW, proj, cst, gamma, _ = case(shape, dtype)
    B, J, Q, rows, n = shape
    freqs = cc.ssq_freqs('log', rows)
    want = run(S, [dev(p) for p in W], [dev(p) for p in dW], cst, proj, gamma, freqs)
    big = torch.zeros((B, rows, n + 3), dtype=dev(W[0]).dtype, device=DEV)
    big[..., 1:-2] = dev(W[0])
    col_slice = big[..., 1:-2]
    assert not col_slice.is_contiguous() and col_slice.data_ptr() != big.data_ptr()
    conj = dev(np.conj(W[1])).conj()
    assert conj.is_conj()
    tall = torch.zeros((B, 2 * rows, n), dtype=conj.dtype, device=DEV)
    tall[:, ::2] = dev(dW[0])
    wider = dev(dW[1].astype(np.complex128 if dtype == 'float32' else np.complex64))
    got = run(S, [col_slice, conj], [tall[:, ::2], wider if dtype == 'float32' else dev(dW[1])], dev(cst), proj,
              gamma, freqs)
    assert torch.equal(got, want)
    assert torch.equal(run(S, W, dW, cst, proj, gamma, freqs), want)              # NumPy planes


def test_abi_refusals_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    lib = _lib.load()
    assert lib.ssq_version() >= 112 and 'ssq_conceft_cwt' in _lib.EXPORTS
    B, J, Q, rows, n = 1, 2, 3, 9, 11
    W, dW, proj, cst = cc.planes((B, J, Q, rows, n), 'float64')
    Wd, dWd, cstd = [dev(p) for p in W], [dev(p) for p in dW], dev(cst)
    kind, p = ssq_grid_params(cc.ssq_freqs('log', rows), True)
    good = dict(W=[t.data_ptr() for t in Wd], dW=[t.data_ptr() for t in dWd], cst=cstd.data_ptr(),
                proj=np.ascontiguousarray(np.stack([proj.real, proj.imag], -1)), batch=B, J=J, Q=Q, rows=rows, n=n,
                gamma=.5, grid=kind, params=_lib.params5(p), Cx=None)
    Cx = torch.full((B, rows, n), -7., dtype=torch.float64, device=DEV)
    good['Cx'] = Cx.data_ptr()

    def call(**kw):
        a = dict(good, **kw)
        ptrs = ctypes.c_void_p * 8
        r = np.ascontiguousarray(a['proj'], dtype=np.float64) if a['proj'] is not None else None
        return lib.ssq_conceft_cwt(_lib.F64, ptrs(*a['W']) if a['W'] is not None else None,
                                   ptrs(*a['dW']) if a['dW'] is not None else None, a['cst'],
                                   r.ctypes.data if r is not None else None, a['Cx'], a['batch'], a['J'], a['Q'],
                                   a['rows'], a['n'], a['gamma'], a['grid'], a['params'], 0, 0, None)
    bad_proj = good['proj'].copy()
    bad_proj[1, 1, 0] = np.inf
    nan_proj = good['proj'].copy()
    nan_proj[2, 0, 1] = np.nan
    refused = [dict(J=0), dict(J=9), dict(Q=0), dict(Q=1025, proj=np.zeros((1025, J, 2))), dict(rows=1), dict(rows=1281),
               dict(batch=0), dict(n=0), dict(batch=1 << 20, rows=64, n=64), dict(W=[Wd[0].data_ptr(), None]),
               dict(dW=[None, dWd[1].data_ptr()]), dict(W=None), dict(dW=None), dict(cst=None), dict(proj=None),
               dict(params=None), dict(Cx=None), dict(proj=bad_proj), dict(proj=nan_proj), dict(gamma=-1.),
               dict(gamma=float('nan')), dict(grid=3), dict(grid=-1)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_conceft_cwt'), (kw, lib.ssq_last_error())
        assert bool((Cx == -7.).all()), kw
    for kind_ok, freqs in ((0, 'log'), (1, 'log-piecewise'), (2, 'linear')):
        kind, p = ssq_grid_params(cc.ssq_freqs(freqs, rows), freqs != 'linear')
        assert kind == kind_ok and call(grid=kind, params=_lib.params5(p)) == 0
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((Cx == -7.).any())


def test_ssq_conceft_is_unchanged(S):
    """The STFT entry next to its new sibling: one case of tests/conceft.py against that module's statement, as
    tests/test_gpu_conceft.py has it."""
    shape, dtype = (2, 3, 4, 33, 50), 'float64'
    V, dV, proj, Sfs = conceft.planes(shape, dtype)
    mags = conceft.magnitudes(V, proj)
    gamma = conceft.above_median(mags)
    near = conceft.near_gamma_columns(mags, gamma)
    for average in ('abs', 'complex'):
        ref = conceft.statement(V, dV, Sfs, proj, gamma, Sfs, True, average)
        Cx = S.conceft_gpu(list(V), list(dV), Sfs, proj, Sfs, gamma, True, average)
        conceft.check('conceft_kernel_next_to_cwt_%s' % average, Cx, ref, near, shape[2], dtype, average)


# ------------------------------------------------------------------------------------------ end to end
def signal(N, B):
    t = np.arange(N) / N
    rng = np.random.default_rng(7)
    x = np.stack([np.cos(2 * np.pi * (.08 * N * t + .05 * N * t * t)) + np.cos(2 * np.pi * .3 * N * t),
                  np.cos(2 * np.pi * .2 * N * t + 1.)]) + .1 * rng.standard_normal((2, N))
    return x[0] if B == 1 else x


@pytest.mark.parametrize('scales', ['log', 'log-piecewise'])
@pytest.mark.parametrize('B', [1, 2], ids=['single', 'batch'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_conceft_cwt_vs_statement_on_its_own_planes(S, dtype, B, scales, N=N):
    import torch
    from ssqueezepy_amd._conceft import draw_projections
    from ssqueezepy_amd._ssq_cwt import _ssq_design
    from ssqueezepy_amd.scales import _process_fs_and_t
    x = signal(N, B)
    wavelet = ('gmw', dict(dtype=dtype))
    kw = dict(wavelet=wavelet, n_tapers=J3, n_proj=Q5, seed=5, scales=scales, nv=NV)
    Cx, Wxs, freqs, sc = S.conceft_cwt(x, **kw)
    rows = len(sc)
    assert Cx.shape == x.shape[:-1] + (rows, N) and len(Wxs) == J3 and not Cx.requires_grad
    assert str(Cx.dtype) == 'torch.' + dtype and freqs[0] > freqs[-1] and len(freqs) == rows
    assert torch.equal(Cx, S.conceft_cwt(x, **kw)[0])                                   # the same seed, the same bits
    assert torch.equal(Cx, S.conceft_cwt(x, **dict(kw, proj=draw_projections(Q5, J3, 5)))[0])
    assert not torch.equal(Cx, S.conceft_cwt(x, **dict(kw, seed=6))[0])
    tapers = S.morse_wavelets(S.Wavelet(wavelet), J3)
    outs = [S.cwt(x, wv, scales=sc, derivative=True) for wv in tapers]
    for got, (Wk, _, _) in zip(Wxs, outs):
        assert torch.equal(got, Wk)
    W, dW = [np.stack([_np(o[i]).reshape(B, rows, N) for o in outs]) for i in (0, 2)]
    _, grid_freqs, const, _, _ = _ssq_design(tapers[0], scales, NV, N, _process_fs_and_t(None, None, N)[0], None, 'peak', True)
    assert np.array_equal(grid_freqs[::-1], freqs)
    proj = conceft.unit_rows(draw_projections(Q5, J3, 5))
    gamma = 10 * float(np.finfo(dtype).eps)
    Tr, Ti, nb = cc.projections(W, dW, const, proj, gamma, grid_freqs)
    near = nb | conceft.near_gamma_columns(conceft.magnitudes(W, proj), gamma)
    ref = cc.average_of(Tr, Ti, True, 'abs')
    cc.check_cwt('conceft_cwt_%s_%d_%s' % (dtype, B, scales), _np(Cx).reshape(B, rows, N), ref, near, Q5, dtype, 'abs')


def test_arguments(S, N=N):
    x = signal(N, 1)
    with pytest.raises(ValueError, match='must be a GMW'):
        S.conceft_cwt(x, 'morlet', nv=NV)
    with pytest.raises(ValueError, match='n_tapers'):
        S.conceft_cwt(x, n_tapers=9, nv=NV)
    with pytest.raises(ValueError, match='average'):
        S.conceft_cwt(x, average='mean', nv=NV)
    Cx, Wxs, freqs, sc = S.conceft_cwt(x, n_tapers=2, n_proj=2, nv=NV, average='complex', astensor=False, flipud=False)
    assert isinstance(Cx, np.ndarray) and np.iscomplexobj(Cx) and isinstance(Wxs[1], np.ndarray)
    assert Cx.shape == Wxs[0].shape == (len(sc), N)


# A tone in white noise, chosen under the emulator on the CPU: there ConceFT's share is 0.6551 and abs(ssq_cwt)'s 0.6470
# within +-2 bins (0.6472 / 0.6397 within +-1, 0.6591 / 0.6515 within +-4; from +-12 on the two are level)
TONE, BAND = .1, 2          # cycles per sample; the band is the tone's bin +- BAND bins


def band_share(C, freqs, fs=1.):
    e = (np.abs(_np(C)).astype(np.float64) ** 2).sum(axis=-1)
    k = int(np.argmin(np.abs(np.log(np.asarray(freqs, dtype=np.float64)) - np.log(TONE * fs))))
    return float(e[k - BAND:k + BAND + 1].sum() / e.sum())


def test_noisy_tone_is_no_less_concentrated_than_ssq_cwt(S, N=N):
    """A tone in white noise at 0 dB: the share of ``|.|^2`` within +-`BAND` bins of the tone's, ConceFT (J = 3,
    Q = 30) against ``abs(ssq_cwt)`` on the same call. Asserted: ConceFT's share is not the lower one. The shares
    themselves are recorded (profiles/conceft_cwt.txt)."""
    rng = np.random.default_rng(2016)
    x = np.cos(2 * np.pi * TONE * np.arange(N)) + np.sqrt(.5) * rng.standard_normal(N)
    kw = dict(nv=NV, fs=1.)
    Cx, _, freqs, _ = S.conceft_cwt(x, 'gmw', 3, 30, **kw)
    Tx, _, freqs2, _ = S.ssq_cwt(x, 'gmw', **kw)
    assert np.array_equal(freqs, freqs2)
    shares = [band_share(Cx, freqs), band_share(Tx, freqs)]
    report_measured('conceft_cwt_noisy_tone_share', conceft_cwt=shares[0], ssq_cwt=shares[1])
    assert shares[0] >= shares[1], shares
