# -*- coding: utf-8 -*-
"""`tssq_stft`, `algos.time_reassign_gpu` and the entry `ssq_time_reassign` (the time-reassigned synchrosqueezing
transform in one kernel).

The oracle of the kernel is `tssq.statement`: the entry's definition in NumPy on separate real float64 arrays, one
ufunc per operation, in the stated order, the scatter as a loop over the source column. The definition has only
basic IEEE operations and a table, and the kernel evaluates the same operations in float64 in the same order, so
the comparison is `==` in both dtypes. What may differ is the branch of a point with ``|Sx|`` within 1e-6
(relative) of `gamma`, where the device's magnitude and libm's `hypot` may disagree: a row with such a point is
left out, and tests/test_tssq_stft_emulated.py asserts that the seeded cases have none.
"""
import ctypes
import os
import numpy as np
import pytest
from conftest import report_measured
import tssq
from tssq import _np, FS

pytestmark = pytest.mark.gpu
DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'
DTYPES = ['float32', 'float64']
SHAPE_IDS = ['one_column', 'short_block', 'one_block', 'block_and_one', 'segment_minus_1', 'segment',
             'segment_plus_1', 'three_segments', 'dmax_0', 'dmax_limit', 'dmax_over_n', 'batch']
CONFLICTS = ['one_cell', 'two_cells', 'straddle']
BATCH_SHAPE = (3, 9, 130, 32, 8, 2)
# end to end
N, N_FFT = 1024, 128


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def limits():
    """The segment length and the largest `dmax` of the library in use."""
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    return lib.ssq_time_reassign_segment(), lib.ssq_time_reassign_max_dmax()


def shape_of(idx, s_rows=3):
    shapes = tssq.shapes(*limits(), s_rows=s_rows)
    assert len(shapes) == len(SHAPE_IDS)
    return shapes[idx]


_CASES = {}


def case(shape, dtype):
    """Planes, a `gamma` midway between two neighbouring samples of ``|Sx|`` at the lower quartile and the points
    near it; made once, nobody writes to them."""
    key = (shape, dtype)
    if key not in _CASES:
        Sx, Vtg = tssq.planes(shape, dtype)
        gamma = tssq.lower_quartile_gamma(Sx)
        _CASES[key] = (Sx, Vtg, gamma, tssq.near_gamma(Sx, gamma))
    return _CASES[key]


_REFS = {}


def reference(shape, dtype, rot='default'):
    key = (shape, dtype, rot)
    if key not in _REFS:
        B, rows, n, n_fft, hop, dmax = shape
        Sx, Vtg, gamma, _ = case(shape, dtype)
        table = {'default': tssq.default_rot(n_fft), 'none': None, 'own': own_rot(n_fft)}[rot]
        _REFS[key] = tssq.statement(Sx, Vtg, table, n_fft, hop, FS / hop, dmax, gamma)
    return _REFS[key]


def own_rot(n_fft):
    rng = np.random.default_rng(n_fft)
    return rng.standard_normal(n_fft) + 1j * rng.standard_normal(n_fft)


def run(S, Sx, Vtg, shape, gamma, rot=None, out=None):
    B, rows, n, n_fft, hop, dmax = shape
    return S.time_reassign_gpu(Sx, Vtg, n_fft, hop, FS, gamma, rot=rot, dmax=dmax, out=out)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------ kernel against statement
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('idx', range(len(SHAPE_IDS)), ids=SHAPE_IDS)
def test_kernel_vs_statement(S, idx, dtype, s_rows=3):
    shape = shape_of(idx, s_rows)
    Sx, Vtg, gamma, near = case(shape, dtype)
    ref = reference(shape, dtype)
    if shape[2] > 1 and shape[5] > 0:
        # terms meet: some cell holds more than one, and some points are dropped on every branch
        ok, c2, _, _ = tssq.terms(Sx, Vtg, None, shape[3], shape[4], FS / shape[4], shape[5], gamma)
        assert 0 < ok.mean() < 1 and (c2[ok] != np.broadcast_to(np.arange(shape[2]), ok.shape)[ok]).any()
    Tx = run(S, Sx, Vtg, shape, gamma)
    assert Tx.dtype == dev(Sx).dtype
    left_out = tssq.check('tssq_kernel_%s_%s' % (SHAPE_IDS[idx], dtype), Tx, ref, near)
    report_measured('tssq_kernel_%s_%s' % (SHAPE_IDS[idx], dtype), rows_left_out=left_out,
                    filled=float((ref != 0).mean()))


@pytest.mark.parametrize('rot', ['none', 'own'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_rotation_tables(S, dtype, rot):
    """``rot=False`` (the entry's NULL: no rotation) and a table of the caller's, on a batch."""
    shape = BATCH_SHAPE
    Sx, Vtg, gamma, near = case(shape, dtype)
    Tx = run(S, Sx, Vtg, shape, gamma, rot=False if rot == 'none' else own_rot(shape[3]))
    tssq.check('tssq_rot_%s_%s' % (rot, dtype), Tx, reference(shape, dtype, rot), near)
    assert not np.array_equal(reference(shape, dtype, rot), reference(shape, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_rotation_index_beyond_32_bits(S, dtype):
    """The kernel's own index arithmetic -- ``a = i hop mod n_fft`` per row, a lane's first ``a (c mod n_fft) mod
    n_fft`` and the step ``+ 64 a mod n_fft`` -- where ``i c hop`` is far beyond 2^32 and `n_fft` is no power of two:
    a hop of 10^12 + 39 on a table of 999 983 entries of the caller's, with `n` past several blocks and a segment so
    that the recurrence wraps many times. Equal to the statement, whose index is Python-exact
    (tests/test_tssq_design.py)."""
    seg, _ = limits()
    n_fft, hop = 999983, 10 ** 12 + 39
    shape = (2, 7, seg + 200, n_fft, hop, 16)
    Sx, Vtg = tssq.planes(shape, dtype)
    gamma = tssq.lower_quartile_gamma(Sx)
    rng = np.random.default_rng(3)
    rot = rng.standard_normal(n_fft) + 1j * rng.standard_normal(n_fft)
    p = tssq.rotation_index(np.arange(7)[:, None], np.arange(shape[2])[None, :], hop, n_fft)
    assert len(np.unique(p)) > shape[2] and int(p.max()) > n_fft // 2
    ref = tssq.statement(Sx, Vtg, rot, n_fft, hop, FS / hop, 16, gamma)
    Tx = S.time_reassign_gpu(Sx, Vtg, n_fft, hop, FS, gamma, rot=rot, dmax=16)
    tssq.check('tssq_rotation_index_%s' % dtype, Tx, ref, tssq.near_gamma(Sx, gamma))
    assert (ref != 0).mean() > .3


# ------------------------------------------------------------------------------------------ order and conflicts
@pytest.mark.parametrize('rot', ['none', 'default'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', CONFLICTS)
def test_order_and_conflicts(S, name, dtype, rot):
    """Many sources of a row meet in one cell -- all of them, alternate lanes in two cells, a run across a block of
    64 and a segment boundary -- with cancelling pairs of terms up to 2^45 among terms of order 1, so that another order
    of the additions gives other bits, after the rounding to float32 too (tests/test_tssq_design.py asserts that the statement can tell)."""
    seg, _ = limits()
    n, dmax, target = tssq.conflict_cases(seg)[name]
    rows, n_fft = 3, 16
    Sx = tssq.wide_range_plane(1, rows, n, dtype, 7, target)
    Vtg = tssq.to_targets(Sx, target)
    table = None if rot == 'none' else tssq.default_rot(n_fft)
    ref = tssq.statement(Sx, Vtg, table, n_fft, 1, FS, dmax, 0.)
    assert (ref != 0).sum() <= rows * (2 if name != 'straddle' else n)
    Tx = S.time_reassign_gpu(Sx, Vtg, n_fft, 1, FS, 0., rot=False if rot == 'none' else None, dmax=dmax)
    tssq.check('tssq_%s_%s_%s' % (name, dtype, rot), Tx, ref, np.zeros(Sx.shape, bool))


# ------------------------------------------------------------------------------------------ other kernel checks
@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_equals_single_calls_and_repeats(S, dtype):
    import torch
    shape = BATCH_SHAPE
    Sx, Vtg, gamma, _ = case(shape, dtype)
    Sd, Vd = dev(Sx), dev(Vtg)
    Tx = run(S, Sd, Vd, shape, gamma)
    assert torch.equal(Tx, run(S, Sd, Vd, shape, gamma))
    for b in range(shape[0]):
        one = run(S, Sd[b], Vd[b], shape, gamma)
        assert one.shape == Tx.shape[1:] and torch.equal(Tx[b], one), b


@pytest.mark.parametrize('dtype', DTYPES)
def test_plane_layouts(S, dtype):
    """Planes handed over as views -- a column slice (strided), a lazy conjugate, a pointer offset by one element,
    NumPy arrays -- and `out=` give the bits of the plain planes; so do pointers that are only 8-byte aligned,
    through the entry itself (the element-load instance in both dtypes)."""
    import torch
    from ssqueezepy_amd import _lib, algos
    shape = BATCH_SHAPE
    B, rows, n, n_fft, hop, dmax = shape
    Sx, Vtg, gamma, _ = case(shape, dtype)
    Sd, Vd = dev(Sx), dev(Vtg)
    want = run(S, Sd, Vd, shape, gamma)
    big = torch.zeros((B, rows, n + 3), dtype=Sd.dtype, device=DEV)
    big[..., 1:-2] = Sd
    col_slice = big[..., 1:-2]
    assert not col_slice.is_contiguous()
    conj = dev(np.conj(Vtg)).conj()
    assert conj.is_conj()
    assert torch.equal(run(S, col_slice, conj, shape, gamma), want)
    flat = torch.zeros(Sd.numel() + 1, dtype=Sd.dtype, device=DEV)
    flat[1:] = Sd.reshape(-1)
    shifted = flat[1:].view(Sd.shape)
    assert shifted.is_contiguous() and shifted.data_ptr() == flat.data_ptr() + Sd.element_size()
    assert torch.equal(run(S, shifted, Vd, shape, gamma), want)
    assert torch.equal(run(S, Sx, Vtg, shape, gamma), want)                  # NumPy planes
    out = torch.full_like(Sd, -7.)
    assert run(S, Sd, Vd, shape, gamma, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError, match='`out`'):
        run(S, Sd, Vd, shape, gamma, out=out[..., ::2])

    # every plane 8 bytes past a 16-byte boundary: real buffers, the planes from their second element on
    lib = _lib.load()
    rdt = torch.float32 if dtype == 'float32' else torch.float64
    step = 8 // (4 if dtype == 'float32' else 8)                           # reals in 8 bytes
    bufs = []
    for src in (Sd, Vd, torch.full_like(Sd, -7.)):
        buf = torch.zeros(2 * src.numel() + step, dtype=rdt, device=DEV)
        buf[step:] = torch.view_as_real(src).reshape(-1)
        assert buf.data_ptr() % 16 == 0
        bufs.append(buf)
    rot = algos.rotation_table(n_fft)
    rc = lib.ssq_time_reassign(_lib.F32 if dtype == 'float32' else _lib.F64, bufs[0].data_ptr() + 8,
                               bufs[1].data_ptr() + 8, rot.data_ptr(), bufs[2].data_ptr() + 8, B, rows, n, n_fft, hop,
                               FS / hop, dmax, float(gamma), algos.stream())
    assert rc == 0, lib.ssq_last_error()
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert torch.equal(bufs[2][step:].reshape(-1, 2), torch.view_as_real(want).reshape(-1, 2))
    assert bool((bufs[2][:step] == 0).all())


def test_abi_refusals_leave_output_unwritten(S):
    import torch
    from ssqueezepy_amd import _lib
    lib = _lib.load()
    assert lib.ssq_version() >= 113 and _lib.ABI_VERSION >= 113 and 'ssq_time_reassign' in _lib.EXPORTS
    seg, max_dmax = limits()
    assert seg >= 64 and seg % 64 == 0 and max_dmax >= 1024
    B, rows, n, n_fft, hop, dmax = shape = (1, 5, 11, 8, 1, 4)
    Sx, Vtg = tssq.planes(shape, 'float64')
    Sd, Vd, rot = dev(Sx), dev(Vtg), dev(tssq.default_rot(n_fft))
    good = dict(Sx=Sd.data_ptr(), Vtg=Vd.data_ptr(), rot=rot.data_ptr(), batch=B, rows=rows, n=n, n_fft=n_fft, hop=hop,
                cps=FS, dmax=dmax, gamma=.5)
    Tx = torch.full((B, rows, n), -7., dtype=torch.complex128, device=DEV)
    good['Tx'] = Tx.data_ptr()

    def call(**kw):
        a = dict(good, **kw)
        return lib.ssq_time_reassign(_lib.F64, a['Sx'], a['Vtg'], a['rot'], a['Tx'], a['batch'], a['rows'], a['n'],
                                     a['n_fft'], a['hop'], a['cps'], a['dmax'], a['gamma'], None)
    refused = [dict(Sx=None), dict(Vtg=None), dict(Tx=None), dict(batch=0), dict(rows=0), dict(n=0),
               dict(batch=1 << 20, rows=64, n=64, n_fft=64), dict(n_fft=0), dict(hop=0), dict(rows=9), dict(dmax=-1),
               dict(dmax=max_dmax + 1), dict(cps=0.), dict(cps=-1.), dict(cps=float('inf')), dict(cps=float('nan')),
               dict(gamma=-1.), dict(gamma=float('nan'))]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.ssq_last_error().decode().startswith('ssq_time_reassign'), (kw, lib.ssq_last_error())
        assert bool((Tx == -7.).all()), kw
    assert call() == 0
    assert call(rot=None, dmax=max_dmax) == 0
    torch.cuda.synchronize() if DEV == 'cuda' else None
    assert not bool((Tx == -7.).any())


@pytest.mark.parametrize('dtype', DTYPES)
def test_row_sums_are_the_kept_coefficients(S, dtype):
    """``Tx.sum(-1)`` is the float64 sum of the rotated kept coefficients of the row, within ``n eps(dtype) sum|Sx|``:
    the transform moves terms along the row and loses none."""
    shape = BATCH_SHAPE
    B, rows, n, n_fft, hop, dmax = shape
    Sx, Vtg, gamma, _ = case(shape, dtype)
    ok, _, vr, vi = tssq.terms(Sx, Vtg, tssq.default_rot(n_fft), n_fft, hop, FS / hop, dmax, gamma)
    want = np.where(ok, vr + 1j * vi, 0.).sum(axis=-1)
    got = _np(run(S, Sx, Vtg, shape, gamma)).astype(np.complex128).sum(axis=-1)
    bound = n * tssq.EPS[dtype] * np.abs(Sx).astype(np.float64).sum(axis=-1)
    report_measured('tssq_row_sums_%s' % dtype, max_err_over_bound=float((np.abs(got - want) / bound).max()))
    assert (np.abs(want) > 0).all() and (np.abs(got - want) <= bound).all()


# ------------------------------------------------------------------------------------------ end to end
def signal(N):
    t = np.arange(N)
    rng = np.random.default_rng(11)
    return np.cos(2 * np.pi * .11 * t) + (np.abs(t - N // 2) < 3) * 4. + .1 * rng.standard_normal(N)


def tau_plane(S, x, g, hop, fs, dtype):
    """The STFT with window ``tau g`` from a plan of its own."""
    import torch
    from ssqueezepy_amd import _stft
    n_fft = len(g)
    tau = (np.arange(n_fft) - n_fft // 2) / fs
    xd = torch.as_tensor(np.asarray(x).astype(dtype)).to(DEV)
    B = 1 if x.ndim == 1 else x.shape[0]
    return _stft.get_stft_plan(x.shape[-1], n_fft, hop, tau * g.astype(dtype).astype('float64'), None, fs, 'reflect',
                               True, dtype, B).execute(xd)['Sx']


@pytest.mark.parametrize('hop', [1, 4])
@pytest.mark.parametrize('dtype', DTYPES)
def test_tssq_stft_is_its_parts(S, dtype, hop, N=N):
    """`Sx` is `stft`'s, `Tx` is `time_reassign_gpu` on it and on a separately executed ``tau g`` plan; a batch is
    its single calls; `get_t`; ``astensor=False``."""
    import torch
    g, fs = tssq.gauss_window(N_FFT), 50.
    x = np.stack([signal(N), signal(N)[::-1].copy()])
    kw = dict(window=g, n_fft=N_FFT, hop_len=hop, fs=fs, dtype=dtype)
    Tx, Sx, Sfs, times = S.tssq_stft(x, **kw)
    n = (N - 1) // hop + 1
    assert Tx.shape == Sx.shape == (2, N_FFT // 2 + 1, n) and not Tx.requires_grad
    assert np.array_equal(Sfs, np.linspace(0, .5 * fs, N_FFT // 2 + 1, dtype=dtype))
    assert times.dtype == np.dtype(dtype) and np.array_equal(times, (np.arange(n) * hop / fs).astype(dtype))
    assert torch.equal(Sx, S.stft(x, **kw))
    Vtg = tau_plane(S, x, g, hop, fs, dtype)
    gamma = 10 * tssq.EPS[dtype]
    assert torch.equal(Tx, S.time_reassign_gpu(Sx, Vtg, N_FFT, hop, fs, gamma))
    for b in range(2):
        one = S.tssq_stft(x[b], **kw)
        assert torch.equal(one[0], Tx[b]) and torch.equal(one[1], Sx[b])
    xt = torch.as_tensor(x[0]).to(DEV).requires_grad_(True)
    Tg, Sg, _, _, t_hat = S.tssq_stft(xt, get_t=True, **kw)
    assert Tg.grad_fn is None and Sg.grad_fn is None and t_hat.grad_fn is None and torch.equal(Tg, Tx[0])
    sx, vt, th = _np(Sx[0]).astype(np.complex128), _np(Vtg[0]).astype(np.complex128), _np(t_hat).astype(np.float64)
    kept = np.abs(sx) >= 2 * gamma
    assert np.isinf(th[np.abs(sx) < .5 * gamma]).all()
    ref = np.broadcast_to(times.astype(np.float64), sx.shape)[kept] + (vt[kept] / sx[kept]).real
    scale = np.abs(vt[kept] / sx[kept]) + times.max()
    assert (np.abs(th[kept] - ref) <= 8 * tssq.EPS[dtype] * scale).all()
    outs = S.tssq_stft(x[0], astensor=False, get_t=True, **kw)
    assert all(isinstance(a, np.ndarray) for a in outs)
    assert np.array_equal(outs[0], _np(Tx[0])) and np.array_equal(outs[1], _np(Sx[0]))


# ------------------------------------------------------------------------------------------ what the transform buys
@pytest.mark.parametrize('hop', [1, 4])
@pytest.mark.parametrize('dtype', DTYPES)
def test_impulse_is_reassigned_to_its_column(S, dtype, hop, N=N):
    """A unit impulse at sample 400: the share of ``|Tx|^2`` in column ``400 / hop`` is >= 0.999, and in every row
    ``|Tx|`` there is the coherent sum ``sum_c |Sx[k, c]|`` over the kept points (1e-4 relative in float32, 1e-10 in
    float64): the rotation lines the terms' phases up."""
    x = np.zeros(N)
    x[400] = 1.
    Tx, Sx, _, _ = S.tssq_stft(x, window=tssq.gauss_window(N_FFT), n_fft=N_FFT, hop_len=hop, fs=1., dtype=dtype)
    Tx, Sx = _np(Tx).astype(np.complex128), _np(Sx).astype(np.complex128)
    col = 400 // hop
    E = np.abs(Tx) ** 2
    share = float(E[:, col].sum() / E.sum())
    coherent = np.where(np.abs(Sx) >= 10 * tssq.EPS[dtype], np.abs(Sx), 0.).sum(axis=-1)
    rel = float((np.abs(np.abs(Tx[:, col]) - coherent) / coherent).max())
    report_measured('tssq_impulse_%s_hop%d' % (dtype, hop), share=share, stft_share=float(
        (np.abs(Sx[:, col]) ** 2).sum() / (np.abs(Sx) ** 2).sum()), coherent_rel_err=rel)
    assert share >= .999
    assert rel <= (1e-4 if dtype == 'float32' else 1e-10)


def test_dispersive_pulse_lands_on_its_group_delay(S, N=N):
    """A pulse with group delay ``300 + 100 f`` samples: the share of the energy, over 0.15 < f < 0.35, within +-1
    column of the true delay. The product's is within 0.01 of the share of a NumPy float64 restatement of the whole
    transform (`tssq.np_tssq`), computed here; ``|stft|^2``'s is below half of it. (A float64 prototype of the
    definition gave 0.995 and 0.153.)"""
    x = tssq.dispersive_pulse(N)
    g = tssq.gauss_window(N_FFT)
    Tx_np, Sx_np = tssq.np_tssq(x, g, 1)
    want = tssq.delay_share(Tx_np, N_FFT, 1)
    for dtype in DTYPES:
        Tx, Sx, _, _ = S.tssq_stft(x, window=g, n_fft=N_FFT, hop_len=1, fs=1., dtype=dtype)
        got, plain = tssq.delay_share(Tx, N_FFT, 1), tssq.delay_share(Sx, N_FFT, 1)
        report_measured('tssq_dispersive_pulse_%s' % dtype, share=got, numpy_share=want, stft_share=plain)
        assert abs(got - want) <= .01, (dtype, got, want)
        assert plain < .5 * want, (dtype, plain, want)
