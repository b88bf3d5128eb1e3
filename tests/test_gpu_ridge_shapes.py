# -*- coding: utf-8 -*-
"""Ridge tracking on the MI355X by row count, on ties and on silent columns (csrc/ssq_ridge.hip).

tests/test_gpu_ridges.py runs smooth random energies, on which every backward step has exactly one matching row.
Here the tracking kernels get `E` directly (tests/ridge_cases.py: ties, all-rows-tie, rounded sums without a match,
and the random kind) at the row counts where `ridge_geometry` changes the forward variant, the LDS tile or the number
of candidate slices, up to the last row count that fits; the elementwise stages are compared with NumPy bit for bit;
`extract_ridges` is compared with the oracle exactly, three ridges deep, dense, sparse and with silent columns.
What the inputs are good for is checked on the CPU by tests/test_ridge_cases_design.py; the same assertions run
under the emulator in tests/test_ridge_kernels_emulated.py."""
import os
import numpy as np
import pytest
import ridge_cases as rc
from conftest import golden
from test_gpu_ridges import _random_tf, _golden_cases

DEV = 'cpu' if os.environ.get('SSQ_EMULATE') == '1' else 'cuda'    # see conftest.compute_module

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


class Device:
    """The driver of tests/ridge_cases.py over device tensors."""

    def __init__(self):
        import torch
        from ssqueezepy_amd import _lib
        self.torch, self.lib, self.F = torch, _lib.load(), {'float32': _lib.F32, 'float64': _lib.F64}

    def dev(self, a):
        return self.torch.tensor(np.asarray(a), device=DEV)

    def host(self, *ts):
        if DEV == 'cuda':
            self.torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in ts]

    def last_error(self):
        return (self.lib.ssq_last_error() or b'').decode()

    def track(self, E, sc, penalty, eps, pe0=None, ridge0=None):
        torch = self.torch
        Ed, scd = self.dev(E), self.dev(sc)
        pe = torch.empty_like(Ed) if pe0 is None else self.dev(pe0)
        ridge = (torch.empty(E.shape[:-2] + E.shape[-1:], dtype=torch.int64, device=DEV) if ridge0 is None
                 else self.dev(ridge0))
        head = (self.F[str(E.dtype)], int(sc.dtype == np.float32), Ed.data_ptr(), pe.data_ptr(), scd.data_ptr(),
                float(penalty), float(eps), E.shape[-2], E.shape[-1], ridge.data_ptr())
        rc_ = (self.lib.ssq_ridge_track(*head, None) if E.ndim == 2
               else self.lib.ssq_ridge_track_batch(*head, E.shape[0], None))
        return (rc_, *self.host(pe, ridge))

    def clear(self, en, ridge, bw, with_e):
        torch = self.torch
        end, rd = self.dev(en), self.dev(ridge)
        r_e = torch.full(ridge.shape, -1., dtype=end.dtype, device=DEV) if with_e else None
        head = (self.F[str(en.dtype)], end.data_ptr(), rd.data_ptr(), float(bw), r_e.data_ptr() if with_e else None,
                en.shape[-2], en.shape[-1])
        rc_ = (self.lib.ssq_ridge_clear(*head, None) if en.ndim == 2
               else self.lib.ssq_ridge_clear_batch(*head, en.shape[0], None))
        return (rc_, *self.host(end, r_e))

    def energy(self, Tf):
        Td = self.dev(Tf)
        rdt = self.torch.float64 if Tf.dtype in (np.complex128, np.float64) else self.torch.float32
        en = self.torch.empty(Tf.shape, dtype=rdt, device=DEV)
        code = self.F[str(en.dtype).replace('torch.', '')]
        rc_ = self.lib.ssq_ridge_energy(code, int(np.iscomplexobj(Tf)), Td.data_ptr(), en.data_ptr(), Tf.shape[0],
                                        Tf.shape[1], None)
        return (rc_, *self.host(en))

    def neglog(self, en, eps):
        end = self.dev(en)
        E = self.torch.empty_like(end)
        rc_ = self.lib.ssq_ridge_neglog(self.F[str(en.dtype)], end.data_ptr(), E.data_ptr(), float(eps), en.shape[0],
                                        en.shape[1], None)
        return (rc_, *self.host(E))


@pytest.fixture(scope='module')
def drv(S):
    return Device()


# ---- tracking, fed E directly ------------------------------------------------------------------------
_TRACK = rc.tracking_cases(rc.SHAPES)


@pytest.mark.parametrize('combo,shape,kind', _TRACK, ids=[rc.case_id(*c) for c in _TRACK])
def test_tracking_by_row_count(drv, orc, combo, shape, kind):
    rc.check_tracking(drv, orc, kind, combo, shape)


@pytest.mark.parametrize('combo', rc.COMBOS, ids=[rc.case_id(c) for c in rc.COMBOS])
def test_tracking_batch_equals_single_calls(drv, orc, combo):
    rc.check_tracking_batch(drv, orc, combo)


# ---- refusal -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('combo', rc.COMBOS, ids=[rc.case_id(c) for c in rc.COMBOS])
def test_one_row_too_many_is_refused_before_any_launch(drv, combo):
    rc.check_refusal(drv, combo)


def test_extract_ridges_refuses_too_many_rows(S):
    from ssqueezepy_amd._lib import SsqError
    na = rc.MAX_ROWS[('float32', 'float32')] + 1
    with pytest.raises(SsqError, match="%d rows do not fit the workgroup's LDS" % na):
        S.extract_ridges(np.ones((na, 3), dtype='complex64'), np.arange(1., na + 1))
    for cdtype, combo in (('float64', ('float64', 'float32')), ('complex128', ('float64', 'float64'))):
        na = rc.MAX_ROWS[combo] + 1
        with pytest.raises(SsqError, match="%d rows do not fit" % na):
            S.extract_ridges(np.ones((na, 3), dtype=cdtype), np.arange(1., na + 1))
    ri = S.extract_ridges(_random_tf(np.random.default_rng(0), 65, 20, 'complex64'), np.arange(1., 66))
    assert ri.shape == (20, 1) and ri.min() >= 0 and ri.max() < 65


# ---- elementwise stages, bit for bit -----------------------------------------------------------------
def _planted(cdtype):
    """0, -0.0, re == im, subnormals, inf, huge / tiny component pairs."""
    rdt = np.zeros(1, cdtype).real.dtype
    fi = np.finfo(rdt)
    sub, big, small = fi.smallest_subnormal, fi.max / 4, fi.tiny * 4
    vals = [(0., 0.), (-0., 0.), (0., -0.), (-0., -0.), (1.5, 1.5), (-3.25, 3.25), (0.1, 0.1), (sub, 0.), (sub, sub),
            (7 * sub, -3 * sub), (fi.tiny, sub), (np.inf, 1.), (-1., np.inf), (np.inf, -np.inf), (-np.inf, 0.),
            (big, small), (small, -big), (big, big), (1e18, 1e-18), (1e-18, 1e18), (small, small), (3., 4.), (1., sub)]
    re, im = np.array(vals, dtype=rdt).T
    if not np.iscomplexobj(np.zeros(1, cdtype)):
        return np.concatenate([re, im])
    z = np.zeros(len(vals), dtype=cdtype)
    z.real, z.imag = re, im
    return z


@pytest.mark.parametrize('cdtype,na,n', [('complex64', 33, 129), ('complex128', 33, 129), ('float32', 33, 129),
                                         ('float64', 33, 129), ('complex64', 65, 65000)])
def test_energy_equals_numpy(drv, cdtype, na, n):
    """`np.abs(Tf)**2`, bit for bit; 65 x 65000 is above 16384 x 256 elements, where the grid-stride loop starts."""
    rng = np.random.default_rng([rc.SEED, na, n])
    Tf = rng.standard_normal((na, n)) * np.exp(rng.uniform(-20, 20, (na, n)))
    if cdtype.startswith('complex'):
        Tf = Tf * np.exp(2j * np.pi * rng.random((na, n)))
    Tf = Tf.astype(cdtype)
    p = _planted(cdtype)
    Tf[2, 3:3 + p.size] = p
    Tf[-1, -p.size:] = p
    with np.errstate(all='ignore'):
        ref = np.abs(Tf)**2
    rc_, en = drv.energy(Tf)
    assert rc_ == 0, drv.last_error()
    assert en.dtype == ref.dtype
    assert np.array_equal(en, ref, equal_nan=True), np.argwhere(~((en == ref) | (np.isnan(en) & np.isnan(ref))))[:8]


@pytest.mark.parametrize('dtype,na,n', [('float32', 65, 300), ('float32', 1, 64), ('float32', 300, 65),
                                        ('float64', 65, 300)])
def test_neglog_against_numpy(drv, dtype, na, n):
    """float32: `-np.log(en / en.max(0) + eps)` bit for bit (np_logf follows NumPy's float32 loop); float64: the
    device's log, within the 4e-13 rule of tests/test_gpu_ridges.py."""
    rng = np.random.default_rng([rc.SEED, na, n])
    en = (rng.random((na, n)) * np.exp(rng.uniform(-30, 0, (na, n)))).astype(dtype)
    en[rng.random((na, n)) < 0.2] = 0                     # exact zeros: log(eps)
    en[0, ::5] = 1.0
    eps = rc.eps_of(dtype)
    with np.errstate(invalid='ignore'):                   # one row: a zero is a silent column, 0 / 0
        ref = -np.log(en / en.max(axis=0) + eps)
    rc_, E = drv.neglog(en, eps)
    assert rc_ == 0, drv.last_error()
    assert E.dtype == ref.dtype
    assert np.array_equal(np.isnan(E), np.isnan(ref)) and np.isnan(ref).any() == (na == 1)
    if dtype == 'float32':
        assert np.array_equal(E, ref, equal_nan=True), float((E != ref).mean())
    else:
        assert np.abs(E - ref).max() <= 4e-13 * max(1., np.abs(ref).max())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_clear_follows_python_slices(drv, dtype):
    rc.check_clear(drv, dtype)


# ---- end to end, three ridges, exact -----------------------------------------------------------------
def _pattern(cdtype, na, n, sparse):
    rng = np.random.default_rng([rc.SEED, na, n])
    Tf = _random_tf(rng, na, n, 'complex128')
    if sparse:
        Tf[np.abs(Tf) < 0.3] = 0
        Tf[:, [n // 3, n - 4]] = 0                        # two silent columns
    return Tf.astype(cdtype) if cdtype.startswith('complex') else np.abs(Tf).astype(cdtype)


def _device_neglog(drv):
    def hook(energy, energy_max, eps):
        rc_, E = drv.neglog(np.ascontiguousarray(energy), eps)
        assert rc_ == 0, drv.last_error()
        return E
    return hook


def _assert_same_ridges(got, ref):
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(got[0], ref[0]), np.argwhere(got[0] != ref[0])[:8]
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2], equal_nan=True)


@pytest.mark.parametrize('bw', [0, 2.5, 4, 300])
@pytest.mark.parametrize('sparse', [False, True], ids=['dense', 'sparse'])
@pytest.mark.parametrize('cdtype', ['complex64', 'float32', 'complex128', 'float64'])
@pytest.mark.parametrize('na,n,transform', [(90, 75, 'cwt'), (200, 40, 'stft')])
def test_three_ridges_equal_the_oracle(S, drv, orc, na, n, transform, cdtype, sparse, bw):
    """complex64 / float32: energy and logarithm are NumPy's, so the oracle as it stands; complex128 / float64: the
    oracle with the device's logarithm of its own energy -- then indices, frequencies and energies are equal."""
    Tf = _pattern(cdtype, na, n, sparse)
    scales = np.exp(np.linspace(0.1, 4.0, na)) if transform == 'cwt' else np.linspace(0, .5, na)
    kw = dict(penalty=2.0 if transform == 'cwt' else 40.0, n_ridges=3, bw=bw, transform=transform, get_params=True)
    got = S.extract_ridges(Tf, scales, **kw)
    hook = None if cdtype in ('complex64', 'float32') else _device_neglog(drv)
    with np.errstate(all='ignore'):
        ref = orc.extract_ridges(Tf, scales, neglog=hook, **kw)
    _assert_same_ridges(got, ref)


@pytest.mark.parametrize('cdtype', ['complex64', 'complex128'])
@pytest.mark.parametrize('where,bw', [('front', 4), ('middle', 4), ('end', 4), (None, 25), ('middle', 25)])
def test_silent_columns_follow_the_numpy_statement(S, drv, cdtype, where, bw):
    """An all-zero column is 0 / 0 in the negative-log energy. np.amin propagates the NaN, the kernel's fmin does
    not; the indices (and with them frequencies and energies) are the reference's all the same. bw = 25 on 40 rows
    silences every column for the later ridges. complex128: the device's logarithm goes through the statement, as
    in the test above."""
    Tf = rc.silent_transform(cdtype, where)
    scales = np.exp(np.linspace(0.1, 3.0, Tf.shape[0]))
    got = S.extract_ridges(Tf, scales, penalty=2.0, n_ridges=3, bw=bw, get_params=True)
    hook = None if cdtype == 'complex64' else _device_neglog(drv)
    ref = rc.extract_ridges_numpy(Tf, scales, penalty=2.0, n_ridges=3, bw=bw, neglog=hook)
    _assert_same_ridges(got, ref)


def test_float32_golden_indices_equal_the_reference_everywhere(S):
    """The float32 cases of tests/golden/ridges.npz: energies and logarithms follow NumPy's operation order, so the
    indices are the reference's at every column of both ridges (tests/test_gpu_ridges.py asks for 99 %)."""
    g = golden('ridges')
    cases = [(k, kw) for k, kw in _golden_cases(g) if k.endswith('/float32')]
    assert len(cases) == 4
    for k, kw in cases:
        ri, rf, re = S.extract_ridges(g[k + '/Tf'], g[k + '/scales'], get_params=True, **kw)
        assert np.array_equal(ri, g[k + '/idx']), (k, float((ri != g[k + '/idx']).mean()))
        assert np.array_equal(rf, g[k + '/f']), k
