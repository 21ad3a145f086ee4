"""CPU-side checks of `lie` (expm / expm_derivatives): signatures, the compat import path, the C ABI's
argument answers, the fixture itself, and the code-object facts of the new kernels."""
import ctypes
import inspect
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT, GOLDEN


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


def test_signatures_match_the_reference():
    """`_impl/expm.py:15` and `:52`: names, order and defaults"""
    from nitorch_fastmath_amd import lie
    assert lie.__all__ == ['expm', 'expm_derivatives']
    s = inspect.signature(lie.expm).parameters
    assert list(s) == ['X', 'basis', 'max_order', 'tol']
    assert (s['basis'].default, s['max_order'].default, s['tol'].default) == (None, 10000, 1e-32)
    s = inspect.signature(lie.expm_derivatives).parameters
    assert list(s) == ['X', 'basis', 'grad_X', 'grad_basis', 'hess_X', 'max_order', 'tol']
    assert [s[k].default for k in list(s)[1:]] == [None, False, False, False, 10000, 1e-32]


def test_compat_resolves_lie():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        importlib.import_module('nitorch_fastmath')
        from nitorch_fastmath.lie import expm, expm_derivatives
        import nitorch_fastmath.lie as nl
        import nitorch_fastmath_amd as N
        assert expm is N.lie.expm and expm_derivatives is N.lie.expm_derivatives and nl is N.lie
        for name in ('logm', 'meanm'):
            with pytest.raises(AttributeError, match='not provide'):
                getattr(nl, name)
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)


def test_facade_refuses_cpu_and_other_dtypes():
    from nitorch_fastmath_amd import lie
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lie.expm(torch.zeros(2, 3, 3))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lie.expm_derivatives(torch.zeros(2, 6), torch.zeros(6, 4, 4), grad_X=True)


def test_abi_answers_without_a_gpu(L):
    """orders without a kernel answer NFM_ESIZE (the facade's torch route), bad arguments NFM_EINVAL / EDTYPE;
    empty batches are a no-op"""
    from nitorch_fastmath_amd import _lib
    op = _lib.Operand(None, 0, 0, 0, 0)
    r = ctypes.byref(op)
    assert L.nfm_lie_expm(_lib.F32, 8, 100, 1e-32, 0, 0, r, r, None) == 0
    assert L.nfm_lie_expm(_lib.F64, 7, 100, 1e-32, 0, 0, r, r, None) == 0
    assert L.nfm_lie_expm(_lib.F64, 8, 100, 1e-32, 0, 0, r, r, None) == -3
    assert L.nfm_lie_expm(_lib.F32, 9, 100, 1e-32, 0, 0, r, r, None) == -3
    assert L.nfm_lie_expm(_lib.F32, 0, 100, 1e-32, 0, 0, r, r, None) == -3
    assert L.nfm_lie_expm(_lib.F32, 3, 100, -1.0, 0, 0, r, r, None) == -1
    assert L.nfm_lie_expm(7, 3, 100, 1e-32, 0, 0, r, r, None) == -2
    assert L.nfm_lie_expm(_lib.F32, 3, 100, 1e-32, 1, 4, r, r, None) == -1          # null pointer, nonempty
    for D in range(1, 5):
        assert L.nfm_lie_expm_frechet(_lib.F64, D, 100, 1e-32, 0, 0, r, r, None, r, None) == 0
        assert L.nfm_lie_expm_frechet(_lib.F32, D, 100, 1e-32, 0, 0, r, r, r, r, None) == 0
    assert L.nfm_lie_expm_frechet(_lib.F64, 5, 100, 1e-32, 0, 0, r, r, None, r, None) == -3


def test_fixture_reference_and_truth_agree_where_the_reference_is_accurate():
    """the reference's plain series is accurate for ||X||_1 <= 0.5 (and the nilpotent inputs, a finite sum);
    at ||X||_1 = 30 in float32 it is not (the issue's table): the fixture records both"""
    g = np.load(os.path.join(GOLDEN, 'lie.npz'))
    worst32 = 0.0
    for dt, eps in (('f32', 2.0 ** -23), ('f64', 2.0 ** -52)):
        for D in range(1, 9):
            x, ref, true, cls = (g[f'{k}_{dt}_{D}'] for k in ('x', 'ref', 'true', 'cls'))
            err = np.abs(ref - true).max((1, 2)) / np.abs(true).max((1, 2))
            ok = (cls > 0) & (cls <= 0.5)
            assert err[ok].max() <= 16 * D * eps, (dt, D, err[ok].max())
            if dt == 'f32':
                worst32 = max(worst32, np.nanmax(np.where(cls == 30, err, 0)))
    assert worst32 > 1e-3            # the inaccuracy this backend does not copy
    for D in (2, 3, 4):
        e = np.abs(g[f'dref_hX_{D}'] - g[f'dtrue_hX_{D}']).max() / np.abs(g[f'dtrue_hX_{D}']).max()
        assert e <= 1e-10, (D, e)
        assert g[f'dref_dB_{D}'].shape[1:] == (D * D, D, D, D, D)


def _census():
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_lie.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_lie_kernels_in_the_census():
    """every (op, dtype, order) the dispatch reaches is compiled, without scratch; 4x4 float32 expm fits
    256 VGPRs (>= 2 waves / SIMD)"""
    rows = _census()
    names = {k['kernel']: k for k in rows}
    assert not [k['kernel'] for k in rows if k['scratch']]
    exp = {n for n in names if 'ExpmOp<' in n}
    fr = {n for n in names if 'ExpmFrechetOp<' in n}
    for D in range(1, 9):
        assert any(f'ExpmOp<float, {D}>' in n for n in exp), D
        assert any(f'ExpmOp<double, {D}>' in n for n in exp) == (D <= 7), D
    for t in ('float', 'double'):
        for D in range(1, 5):
            for depth in (1, 2):
                assert any(f'ExpmFrechetOp<{t}, {D}, {depth}>' in n for n in fr), (t, D, depth)
    assert not any('ExpmFrechetOp<float, 5' in n for n in fr)
    f4 = [names[n] for n in exp if 'ExpmOp<float, 4>' in n]
    assert f4 and max(k['vgpr'] for k in f4) <= 256
