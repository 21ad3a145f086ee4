"""The matrix-core route of realtransforms without a GPU: the two entry points are exported and declared, and
nfm_rt_transform_mm refuses bad calls with the status codes of nfm_rt_transform before any launch."""
import ctypes
import os
import re
import pytest
from conftest import ROOT


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_declared(L):
    from nitorch_fastmath_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for name in ('nfm_rt_transform_mm', 'nfm_rt_mm_max_len'):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    assert _lib.SIGNATURES['nfm_rt_transform_mm'] == _lib.SIGNATURES['nfm_rt_transform']
    assert 'NFM_RT_MAX_N 256' in header


def test_abi_refuses_bad_calls_before_any_launch(L):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(dtype=0, kind=0, type=2, norm=0, tr=0, N=4, outer=2, inner=2, x=p, out=p):
        return L.nfm_rt_transform_mm(dtype, kind, type, norm, tr, N, outer, inner, x, out, None)
    assert call(dtype=7, N=-1, x=None) == -2                      # dtype first
    assert call(dtype=2) == -2
    assert call(N=-1, kind=9) == -1 and call(outer=-1) == -1 and call(inner=-1) == -1
    assert call(kind=2) == -1 and call(kind=-1) == -1 and call(type=0) == -1 and call(type=4) == -1
    assert call(norm=4) == -1 and call(norm=-1) == -1 and call(tr=2) == -1 and call(tr=-1) == -1
    assert call(N=0) == -1
    assert call(kind=0, type=1, N=1) == -1                        # DCT-I of one point
    assert call(N=4, outer=1 << 40, inner=1 << 40, x=None) == -3  # element count past int64, before the pointers
    assert call(N=257, x=None) == -100                            # past NFM_RT_MAX_N, before the pointers
    assert call(dtype=1, N=257, x=None) == -100
    assert call(x=None) == -1 and call(out=None) == -1            # null pointer, non-empty batch
    assert call(x=p + 2) == -4 and call(out=p + 4, dtype=1) == -4  # misaligned
    assert call(outer=0, x=None, out=None) == 0 and call(inner=0, x=None, out=None) == 0
    assert call(N=256, outer=0, x=None, out=None) == 0            # every length up to 256 is served


def test_routing_cap_and_version(L):
    assert L.nfm_rt_mm_max_len(0) in (64, 128, 256)
    assert L.nfm_rt_mm_max_len(1) in (64, 128, 256)
    assert L.nfm_rt_mm_max_len(7) == -2
    assert L.nfm_version() == 5


def test_facade_reads_the_cap(L):
    import torch
    from nitorch_fastmath_amd import realtransforms as RT
    assert RT.mm_max_len(torch.float32) == L.nfm_rt_mm_max_len(0)
    assert RT.mm_max_len(torch.float64) == L.nfm_rt_mm_max_len(1)
    assert RT.mm_max_len(torch.float16) == 0
    x = torch.zeros(3, 200)
    assert RT._route(x, 200, False) == 'torch'                    # CPU tensors stay on the composition
