# -*- coding: utf-8 -*-
"""The fused float32 STFT kernels BY WINDOW LENGTH (tests/stft_lengths.py has the table, the float64 statement and the
per-column check, and says what each length is there for): every radix of the mixed-radix kernel first, in the
middle, last and alone; both sides of every edge of G, the frames per workgroup; the lengths that fill the epilogue's
register arrays; the grid's remap per XCD against the statement; a frame's bits wherever it sits; the power-of-two
kernel's five lengths through the same check.

Every statement about what ran reads a fact: `plan.algo` and `ssq_stft_generic_shape` (the radices and G of the
length, no device call), held against the table -- which tests/test_stft_lengths_design.py holds against a Python
restatement of the planning rule. Inputs: `two_chirps` in float32. tests/test_stft_lengths_emulated.py runs a subset
over the CPU emulation of the kernels; profiles/stft_lengths.txt has the measured figures."""
import numpy as np
import pytest
from conftest import assert_tx_vs_oracle, report_measured, tile_order
import stft_lengths as L

pytestmark = pytest.mark.gpu
GAMMA = 10 * L.EPS32
MIXED = tuple(n for n, e in L.LENGTHS.items() if e.radix)


@pytest.fixture(scope='module')
def S():
    from conftest import compute_module
    yield from compute_module()


def lib():
    from ssqueezepy_amd import _lib
    return _lib.load(build_if_missing=False)


def check_length(S, n_fft):
    """Route, radices and G of `n_fft` against the table, then the per-column bound at its two shapes."""
    e = L.LENGTHS.get(n_fft)
    if e is None:                                   # the power-of-two kernel
        algo, G = 'fused', L.POW2[n_fft]
        assert L.query(lib(), n_fft) is None
    elif e.radix is None:
        algo, G = 'rocfft', None
        assert L.query(lib(), n_fft) is None
    else:
        algo, G = 'fused-mixed-radix', e.G
        assert L.query(lib(), n_fft) == (e.radix, e.G), (n_fft, L.query(lib(), n_fft))
        if n_fft in L.FULL_EPILOGUE:
            assert L.epilogue_points(n_fft, G) == L.GEN_MAX_EPI
    worst = {}
    for sh in L.shapes(n_fft, G):
        x = L.signal(sh['N'], seed=n_fft + sh['hop'])
        f = L.check_columns(S, x, n_fft, sh['hop'], sh['modulated'], sh['padtype'], algo, (n_fft, sh))
        for k in ('Sx', 'dSx'):
            worst[k] = max(worst.get(k, 0.), f[k])
    report_measured('stft_lengths', n_fft=n_fft, algo=algo, G=G or 0, e_Sx=worst['Sx'], e_dSx=worst['dSx'])


@pytest.mark.parametrize('n_fft', sorted(L.LENGTHS))
def test_stft_columns_by_length(S, n_fft):
    """Sx and dSx of every length of the table, column by column, at a shape whose last workgroup holds one frame
    (modulated) and at hop 1 with zero padding (not modulated)."""
    check_length(S, n_fft)


@pytest.mark.parametrize('n_fft', sorted(L.POW2))
def test_stft_columns_power_of_two_kernel(S, n_fft):
    """stft_fused_kernel's five lengths through the same check at the same partial-last-group shapes (its G:
    4096 / n_fft frames per workgroup)."""
    check_length(S, n_fft)


def ssq_routes(S, orc, n_fft, flipud=False):
    """`ssq_stft` without dSx three ways -- Tx summed in the kernel, the 2-byte bin map with the separate pass
    (`SSQ_DEBUG_STFT_FUSED_TX=0`, read at every call), the ordered sums (dSx kept) --: the same Sx bit for bit, the
    ordered Tx `==` the oracle's reassignment of the device's own Sx, dSx, the other two against it as
    test_fused_stft_every_size holds them; Sx to 1e-5 of the oracle's largest magnitude."""
    import os
    from ssqueezepy_amd import _stft
    from ssqueezepy_amd.ssqueezing import ssq_grid_params
    from pipeline import oracle_ssq_stft
    e = L.LENGTHS[n_fft]
    sh = L.shapes(n_fft, e.G)[0]
    x = L.signal(sh['N'], seed=3 * n_fft)
    kw = dict(window=L.window_spec(n_fft), n_fft=n_fft, hop_len=sh['hop'], dtype='float32', flipud=flipud,
              astensor=False)
    saved = os.environ.pop('SSQ_DEBUG_STFT_FUSED_TX', None)
    _stft._PLAN_CACHE.clear()
    try:
        Tf, Sf, sf, Sfs = S.ssq_stft(x, **kw)
        assert list(_stft._PLAN_CACHE.values())[-1].algo == 'fused-mixed-radix'
        os.environ['SSQ_DEBUG_STFT_FUSED_TX'] = '0'
        Tk, Sk, *_ = S.ssq_stft(x, **kw)
        del os.environ['SSQ_DEBUG_STFT_FUSED_TX']
        To, So, _, _, dSo = S.ssq_stft(x, get_dWx=True, **kw)
    finally:
        os.environ.pop('SSQ_DEBUG_STFT_FUSED_TX', None)
        if saved is not None:
            os.environ['SSQ_DEBUG_STFT_FUSED_TX'] = saved
        _stft._PLAN_CACHE.clear()
    assert Sf.shape == (n_fft // 2 + 1, sh['n_hops'])
    assert np.array_equal(Sf, So) and np.array_equal(Sk, So), n_fft
    _, p = ssq_grid_params(Sfs, False)
    ref = orc.ssqueeze(So, dSo, 'linear', p, Sfs[1] - Sfs[0], GAMMA, flipud, Sfs=Sfs, typing=0)
    assert np.array_equal(To, ref), n_fft
    assert np.abs(ref).max() > 0
    assert_tx_vs_oracle(Tf, ref, what=(n_fft, 'fused'))
    assert_tx_vs_oracle(Tk, ref, what=(n_fft, 'bin map'))
    win, dwin = S.get_window(L.window_spec(n_fft), n_fft, n_fft, derivative=True, dtype='float32')
    Sr, dSr = orc.stft(x, win, dwin, n_fft, sh['hop'], fs=1., modulated=True, derivative=True, padtype='reflect')
    assert np.abs(So - Sr).max() <= 1e-5 * np.abs(Sr).max() and np.abs(dSo - dSr).max() <= 1e-5 * np.abs(dSr).max()


@pytest.mark.parametrize('n_fft', sorted(MIXED))
def test_ssq_stft_three_tx_routes_by_length(S, orc, n_fft):
    ssq_routes(S, orc, n_fft)


@pytest.mark.parametrize('n_fft', [31, 4992])
def test_ssq_stft_three_tx_routes_flipud(S, orc, n_fft):
    """... with `flipud` at G = 16 and at G = 1."""
    assert L.LENGTHS[n_fft].G == (16 if n_fft == 31 else 1)
    ssq_routes(S, orc, n_fft, flipud=True)


# (n_fft, hop, n_hops, workgroups per signal)
REMAP = [(60, 1, 1093, 69), (598, 7, 265, 67), (2499, 50, 67, 67), (60, 1, 1152, 72), (60, 1, 1001, 63)]


def check_remap(S, n_fft, hop, n_hops, nb):
    """A batch of three through a grid of `nb` workgroups per signal against the statement, every column of every
    signal: from 64 on the grid is padded to a multiple of 8 and the workgroups are remapped per XCD (69, 67: padded
    blocks that return early, at G = 16, 4, 1; 72: none padded; 63: the last grid that is not remapped)."""
    radix, G = L.query(lib(), n_fft)
    assert -(-n_hops // G) == nb and (nb >= L.XCD_FROM or nb == L.XCD_FROM - 1)
    N = (n_hops - 1) * hop + 1
    x = L.signal(N, seed=n_fft + nb, B=3)
    f = L.check_columns(S, x, n_fft, hop, True, 'reflect', 'fused-mixed-radix', (n_fft, hop, n_hops))
    report_measured('stft_lengths_remap', n_fft=n_fft, nb=nb, G=G, e_Sx=f['Sx'], e_dSx=f['dSx'])


@pytest.mark.parametrize('n_fft,hop,n_hops,nb', REMAP)
def test_xcd_remap_vs_statement(S, n_fft, hop, n_hops, nb):
    check_remap(S, n_fft, hop, n_hops, nb)


def check_position(S, n_fft, shift):
    """Mixed-radix kernel: a frame's bits do not depend on where it sits. x2 = x moved left by `shift` hops: column
    c + shift of stft(x) and column c of stft(x2) hold the same samples wherever neither touches the padding -- in
    another lane g of the workgroup, and, for the frames near a multiple of G, in another workgroup. Nothing in the
    kernel's arithmetic reads g or the workgroup's index (loads, twiddles and stores are indexed by them, values are
    not), so Sx and dSx are equal bit for bit."""
    e = L.LENGTHS[n_fft]
    hop, G = 3, e.G
    N = n_fft + hop * (3 * G + 2 + shift)
    xl = L.signal(N + shift * hop, seed=n_fft)
    x, x2 = xl[:N].copy(), xl[shift * hop:].copy()
    n1 = (n_fft - 1) - (n_fft - 1) // 2
    S1, D1, a1 = L.run_stft(S, x, n_fft, hop, True, 'reflect')
    S2, D2, a2 = L.run_stft(S, x2, n_fft, hop, True, 'reflect')
    assert a1 == a2 == 'fused-mixed-radix' and S1.shape == S2.shape
    c = np.arange(S1.shape[1] - shift)
    inner = (c * hop >= n1) & ((c + shift) * hop - n1 + n_fft <= N)       # frame c of x2 and frame c + shift of x
    c = c[inner]
    assert len(c) >= 3 * G and len(set((c // G).tolist())) >= 3           # workgroups apart
    assert ((c % G) != ((c + shift) % G)).any() and ((c // G) != ((c + shift) // G)).any()
    assert np.abs(S1[:, c + shift]).max() > 0
    assert np.array_equal(S1[:, c + shift], S2[:, c]) and np.array_equal(D1[:, c + shift], D2[:, c]), (n_fft, shift)


@pytest.mark.parametrize('n_fft,shift', [(156, 1), (312, 3), (598, 1), (2187, 3)])
def test_frame_bits_do_not_depend_on_position(S, n_fft, shift):
    assert L.LENGTHS[n_fft].G == {156: 16, 312: 8, 598: 4, 2187: 2}[n_fft]
    check_position(S, n_fft, shift)
