# -*- coding: utf-8 -*-
"""The device-table cache of `ssq_cwt2_phase` and `ssq_conceft` (csrc/ssq_common.h: DeviceTableCache) with the
product's own host code under the CPU emulator (tests/emu/, tests/emu_backend.py): the case of
tests/test_gpu_table_cache.py, run as it is. CPU-only."""
import pytest
import emu_backend
import test_gpu_table_cache as T


@pytest.fixture(scope='module')
def S():
    if not emu_backend.available():
        pytest.skip("no clang++ under $ROCM_PATH/lib/llvm/bin")
    with emu_backend.emulated() as mod:
        yield mod


@pytest.mark.parametrize('entry', ['ssq_cwt2_phase', 'ssq_conceft'])
def test_more_tables_than_the_cache_keeps(S, entry):
    T.test_more_tables_than_the_cache_keeps(S, entry)
