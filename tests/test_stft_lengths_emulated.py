# -*- coding: utf-8 -*-
"""The window-length tests of tests/test_gpu_stft_lengths.py with the product's own kernels and host code under the
CPU emulator (tests/emu/, tests/emu_backend.py), run as they are: the per-column check on the single passes, both sides of
every G edge, 961 (the same radix first and last), 1798 (29 in the middle), 4374 (eight passes) and 4992 (the LDS and
the epilogue full) in the emulator's default order and with the wavefronts of a workgroup shuffled after every barrier
and the lanes reversed, on the rest of the table in the default order; the three Tx routes on a few lengths; the
remapped grids at G = 16 and G = 1; a frame's bits by position. CPU-only."""
import pytest
import block_builds
import stft_lengths as L
import test_gpu_stft_lengths as T


@pytest.fixture(scope='module', params=['default-order', 'shuffle-reverse'])
def S(request, tmp_path_factory):
    yield from block_builds.emulated_module(request.param, tmp_path_factory, 'libssq_hip_emu_stft_lengths.so')


@pytest.fixture(scope='module')
def S0():
    import emu_backend
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.mark.parametrize('n_fft', sorted(set(L.EMULATED) - {4998}))
def test_stft_columns_by_length(S, n_fft):
    T.check_length(S, n_fft)


@pytest.mark.parametrize('n_fft', sorted(set(L.LENGTHS) - set(L.EMULATED) - {5000}) + [4998])
def test_stft_columns_rest_of_the_table(S0, n_fft):
    """... and the other lengths in the default order alone (4998: the emulator's rocFFT is a plain DFT, 14 s; 5000 is
    the device module's)."""
    T.check_length(S0, n_fft)


@pytest.mark.parametrize('n_fft', [128, 2048])
def test_stft_columns_power_of_two_kernel(S0, n_fft):
    T.check_length(S0, n_fft)


@pytest.mark.parametrize('n_fft,flipud', [(2, False), (29, False), (31, True), (160, False), (961, False),
                                          (1248, False), (2496, False), (4992, True)])
def test_ssq_stft_three_tx_routes(S0, orc, n_fft, flipud):
    T.ssq_routes(S0, orc, n_fft, flipud)


@pytest.mark.parametrize('n_fft,hop,n_hops,nb', [T.REMAP[0], T.REMAP[2], T.REMAP[4]])
def test_xcd_remap_vs_statement(S0, n_fft, hop, n_hops, nb):
    T.check_remap(S0, n_fft, hop, n_hops, nb)


@pytest.mark.parametrize('n_fft,shift', [(156, 1), (598, 1)])
def test_frame_bits_do_not_depend_on_position(S0, n_fft, shift):
    T.check_position(S0, n_fft, shift)
