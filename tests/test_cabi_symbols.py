# -*- coding: utf-8 -*-
"""The C-ABI shared library must build for gfx950 without a GPU, load, and export
every symbol include/ssq_hip.h declares (no compute calls here). CPU-only."""
import os
import re
import ctypes
from conftest import ROOT


def _declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'ssq_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(ssq_[a-z0-9_]+)\s*\(', txt)))


def test_library_builds_loads_and_exports_header_symbols():
    from ssqueezepy_amd import build, _lib
    path = build.build(verbose=False)
    assert os.path.isfile(path)
    lib = ctypes.CDLL(path)
    declared = _declared_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), "missing export: " + name
    # the ctypes binding covers the same set
    assert sorted(_lib.EXPORTS) == declared
    lib.ssq_version.restype = ctypes.c_int
    assert lib.ssq_version() >= 105


def test_stft_generic_shape_needs_no_device():
    """`ssq_stft_generic_shape` (ABI 116): what the mixed-radix STFT kernel runs for a window length, answered on the
    host -- the reference's published shape, a power of two of the other kernel, a prime above 31, the first length
    past the LDS (tests/test_stft_lengths_design.py: every length against the rule)."""
    from ssqueezepy_amd import build, _lib
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.ssq_version.restype = ctypes.c_int
    assert lib.ssq_version() >= 116 and _lib.ABI_VERSION >= 116 and 'ssq_stft_generic_shape' in _lib.EXPORTS
    fn = lib.ssq_stft_generic_shape
    fn.restype, fn.argtypes = _lib._PROTOS['ssq_stft_generic_shape']
    radix, npass, G = (ctypes.c_int * 10)(), ctypes.c_int(), ctypes.c_int()
    assert fn(598, radix, ctypes.byref(npass), ctypes.byref(G)) == 1
    assert (list(radix), npass.value, G.value) == ([2, 13, 23] + [0] * 7, 3, 4)
    assert fn(4992, radix, ctypes.byref(npass), ctypes.byref(G)) == 1
    assert (list(radix), npass.value, G.value) == ([16, 8, 3, 13] + [0] * 6, 4, 1)
    for n in (256, 97, 4998, 0):
        assert fn(n, radix, ctypes.byref(npass), ctypes.byref(G)) == 0
        assert (list(radix), npass.value, G.value) == ([0] * 10, 0, 0)


def test_reassign_route_and_bins_entry_need_no_device():
    """`ssq_reassign_route` and `ssq_indexed_sum_bins` (ABI 118): the route of the reassignment kernels for a shape,
    answered on the host -- both sides of the float32 32- to 16-column edge, the unordered float64 tile's last row
    count, the global kernel, a refusal (tests/test_reassign_rows_design.py: every row count against the rule)."""
    from ssqueezepy_amd import build, _lib
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.ssq_version.restype = ctypes.c_int
    assert lib.ssq_version() >= 118 and _lib.ABI_VERSION >= 118
    assert 'ssq_reassign_route' in _lib.EXPORTS and 'ssq_indexed_sum_bins' in _lib.EXPORTS
    assert hasattr(lib, 'ssq_indexed_sum_bins')
    fn = lib.ssq_reassign_route
    fn.restype, fn.argtypes = _lib._PROTOS['ssq_reassign_route']
    kernel, cols, waves = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out = (ctypes.byref(kernel), ctypes.byref(cols), ctypes.byref(waves))
    names = _lib.REASSIGN_KERNELS
    assert names == ('tile16', 'tile', 'f64', 'global')
    for args, want in (((_lib.F32, _lib.BIN_FROM_DWX, 320, 100, 0, 0), ('tile16', 32, 4)),
                       ((_lib.F32, _lib.BIN_FROM_DWX, 321, 100, 0, 0), ('tile16', 16, 2)),
                       ((_lib.F64, _lib.BIN_FROM_KIDX, 1280, 100, 0, 0), ('f64', 8, 8)),
                       ((_lib.F64, _lib.BIN_FROM_KIDX, 1280, 100, 1, 0), ('tile', 8, 1)),
                       ((_lib.F64, _lib.BIN_FROM_KIDX, 1280, 100, 0, 1), ('tile', 8, 1)),
                       ((_lib.F32, _lib.BIN_FROM_W, 5121, 100, 0, 0), ('global', 1, 4)),
                       ((_lib.F32, _lib.BIN_FROM_W, 640, 1 << 22, 0, 0), ('tile', 16, 1))):
        assert fn(*args, *out) == 0
        assert (names[kernel.value], cols.value, waves.value) == want, args
    assert fn(7, 0, 10, 10, 0, 0, *out) == -1 and (kernel.value, cols.value, waves.value) == (-1, 0, 0)


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'ssqueezepy_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.inl')):
                src = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in src and 'from oracle' not in src, f
                assert 'libssq_oracle' not in src, f


def test_compute_layer_fails_loudly_without_gpu():
    import torch
    import pytest
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import numpy as np
    from ssqueezepy_amd import cwt
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cwt(np.random.randn(512), 'gmw', scales='log')


def test_c_client_against_emulated_library(tmp_path):
    """tests/cabi/cabi_smoke.c (the plain-C client of include/ssq_hip.h that the GPU suite
    runs against libssq_hip.so) linked against the host build of the same sources
    (tests/emu/): the C ABI exercised end to end without a GPU."""
    import emu_backend
    from test_gpu_cabi_c import build_and_run
    if not emu_backend.available():
        import pytest
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    lib = emu_backend.build()
    build_and_run(tmp_path, os.path.dirname(lib), os.path.basename(lib))
