"""realtransforms without a GPU: the dense matrices of tests/_realtransforms_ref.py against the reference's
recorded ones and against scipy, the public surface, the argument checks of the C ABI, the per-line routine on
the CPU (nfm_rt_transform_host) and the torch composition that serves long axes and CPU tensors.

Bounds.  Against the dense float64 matrix: `_realtransforms_ref.bound`, (N + 6) eps sum |M_kn| |x_n| plus the
smallest normal number.  Against the fixture (the reference's float64 FFT composition, whose matrices agree
with the dense ones to FIXTURE_TOL = 1e-13 per entry -- the first test -- but not to a relative error, e.g. 1e-16
where the matrix has a zero) the fixture's own error is allowed on top: FIXTURE_TOL sum |x_n|.  The torch
composition is an FFT as well: its error is relative to the norm of a line, not to the terms of one output,
so it is held to the bound on dense random inputs and to FIXTURE_TOL-sized errors per unit of sum |x_n| in
float64 on the unit impulses."""
import ctypes
import inspect
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT, GOLDEN
import _realtransforms_ref as R

FIXTURE_TOL = 1e-13
DTYPES = {np.float32: 0, np.float64: 1}


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'realtransforms.npz'))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


def cases(ns=None):
    for kind in R.KINDS:
        for type in R.TYPES:
            for norm in R.NORMS:
                for direction in ('fwd', 'inv'):
                    yield kind, type, norm, direction


def dense(kind, type, norm, direction, N):
    return (R.inverse_matrix if direction == 'inv' else R.matrix)(kind, type, norm, N)


def host(L, kind, type, norm, transpose, x, axis, dtype):
    """nfm_rt_transform_host along `axis` of a C-contiguous array"""
    x = np.ascontiguousarray(x, dtype=dtype)
    out = np.empty_like(x)
    N = x.shape[axis]
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    rc = L.nfm_rt_transform_host(DTYPES[dtype], R.KINDS.index(kind), type, R.NORMS.index(norm), transpose, N, outer,
                                 inner, x.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def test_dense_matrices_equal_the_recorded_ones(fx):
    seen = 0
    for kind, type, norm, direction in cases():
        for N in fx['ns']:
            key = f'mat_{kind}_{type}_{norm}_{direction}_{N}'
            if key not in fx:
                assert kind == 'dct' and type == 1 and N == 1, key
                continue
            assert np.abs(dense(kind, type, norm, direction, int(N)) - fx[key]).max() <= FIXTURE_TOL, key
            seen += 1
    assert seen == 2 * 3 * 4 * 2 * len(fx['ns']) - 8


def test_reference_raises_only_for_one_point_dct1(fx):
    rows = [r.split() for r in fx['raises']]
    assert len(rows) == 8 and all(r[:2] == ['dct', '1'] and r[4] == '1' for r in rows)
    assert {r[5] for r in rows} <= {'ZeroDivisionError', 'RuntimeError'}
    with pytest.raises(ValueError):
        R.matrix('dct', 1, 'backward', 1)


def test_standard_norms_equal_scipy():
    sf = pytest.importorskip('scipy.fft')
    for kind in R.KINDS:
        for type in R.TYPES:
            for norm in ('backward', 'forward', 'ortho'):
                for N in (2, 3, 8, 17):
                    want = getattr(sf, kind)(np.eye(N), type=type, norm=norm, axis=0)
                    assert np.abs(R.matrix(kind, type, norm, N) - want).max() <= FIXTURE_TOL, (kind, type, norm, N)
                    want = getattr(sf, 'i' + kind)(np.eye(N), type=type, norm=norm, axis=0)
                    assert np.abs(R.inverse_matrix(kind, type, norm, N) - want).max() <= FIXTURE_TOL


def test_ortho_scipy_is_its_own_convention_for_dst_2_and_3():
    for type in (2, 3):
        a, b = R.matrix('dst', type, 'ortho', 8), R.matrix('dst', type, 'ortho_scipy', 8)
        assert np.abs(a - b).max() > 0.1
        assert np.abs(a @ a.T - np.eye(8)).max() < 1e-14           # 'ortho' is orthogonal ...
        assert np.abs(b @ b.T - np.eye(8)).max() > 0.1             # ... 'ortho_scipy' is not
        assert np.array_equal(R.matrix('dct', type, 'ortho', 8), R.matrix('dct', type, 'ortho_scipy', 8))


def test_public_surface_matches_upstream():
    from nitorch_fastmath_amd import realtransforms as RT
    import nitorch_fastmath_amd as N
    assert RT.__all__ == ['dct', 'dst', 'idct', 'idst', 'dctn', 'dstn', 'idctn', 'idstn']
    assert N.realtransforms is RT
    table = {name: (['x', 'dim', 'norm', 'type'], (None if name.endswith('n') else -1, 'backward', 2))
             for name in RT.__all__}
    for name, (params, defaults) in table.items():
        sig = inspect.signature(getattr(RT, name))
        assert list(sig.parameters) == params, name
        assert tuple(sig.parameters[p].default for p in params[1:]) == defaults, name


def test_compat_package_serves_realtransforms():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        nf = importlib.import_module('nitorch_fastmath')
        mod = importlib.import_module('nitorch_fastmath.realtransforms')
        from nitorch_fastmath import dctn, idstn  # noqa: F401
        import nitorch_fastmath_amd as N
        assert mod is N.realtransforms and nf.dctn is N.realtransforms.dctn and nf.dst is N.realtransforms.dst
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)


def test_abi_refuses_bad_calls_before_any_launch(L):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    cap32, cap64 = L.nfm_rt_max_len(0), L.nfm_rt_max_len(1)
    assert 64 <= cap32 <= 256 and 64 <= cap64 <= 256 and L.nfm_rt_max_len(7) == -2
    for fn, tail in ((L.nfm_rt_transform, (None,)), (L.nfm_rt_transform_host, ())):
        def call(dtype=0, kind=0, type=2, norm=0, tr=0, N=4, outer=2, inner=2, x=p, out=p):
            return fn(dtype, kind, type, norm, tr, N, outer, inner, x, out, *tail)
        assert call(dtype=7, N=-1, x=None) == -2                      # dtype first
        assert call(N=-1, kind=9) == -1 and call(outer=-1) == -1 and call(inner=-1) == -1
        assert call(kind=2) == -1 and call(type=0) == -1 and call(type=4) == -1
        assert call(norm=4) == -1 and call(norm=-1) == -1 and call(tr=2) == -1
        assert call(N=0) == -1
        assert call(kind=0, type=1, N=1) == -1                        # DCT-I of one point
        assert call(N=4, outer=1 << 40, inner=1 << 40, x=None) == -3  # element count past int64, before the pointers
        assert call(N=257, x=None) == -100                            # past every cap, before the pointers
        assert call(x=None) == -1 and call(out=None) == -1            # null pointer, non-empty batch
        assert call(x=p + 2) == -4 and call(out=p + 4, dtype=1) == -4
        assert call(outer=0, x=None, out=None) == 0 and call(inner=0, x=None, out=None) == 0
    assert L.nfm_rt_transform(0, 0, 2, 0, 0, cap32 + 1, 1, 1, None, None, None) == -100
    assert L.nfm_rt_transform(1, 0, 2, 0, 0, cap64 + 1, 1, 1, None, None, None) == -100
    assert b'longer' in L.nfm_strerror(-100)
    assert L.nfm_version() == 5


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_routine_gives_the_matrix_columns(L, dtype):
    """unit impulses along axis 0 of an (N, N) array (lines a stride apart: the `inner > 1` addressing), every
    kind, type, norm and transpose setting, at lengths on both sides of the blocks of 8 outputs, up to 256"""
    worst = 0.0
    for kind in R.KINDS:
        for type in R.TYPES:
            for norm in R.NORMS:
                for N in (1, 2, 3, 7, 8, 9, 16, 17, 33, 64, 256):
                    if kind == 'dct' and type == 1 and N == 1:
                        continue
                    M = R.matrix(kind, type, norm, N)
                    eye = np.eye(N, dtype=dtype)
                    for tr in (0, 1):
                        want = M.T if tr else M
                        got = host(L, kind, type, norm, tr, eye, 0, dtype)
                        r = R.ratio(got, want, R.bound(want, eye, dtype, axis=0))
                        worst = max(worst, r)
                        assert r <= 1, (kind, type, norm, N, tr, r)
                        assert np.all(got[want == 0] == 0), 'zeros of the matrix are exact zeros'
    print(f'worst fraction of the bound ({np.dtype(dtype).name}): {worst:.3f}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_routine_reproduces_the_fixture(L, fx, dtype):
    for kind, type, norm, direction in cases():
        rk = (R.FLIPTYPE[type], R.FLIPNORM[norm]) if direction == 'inv' else (type, norm)
        for tag in ('f32', 'f64'):
            x = fx[f'x_{tag}']
            if dtype == np.float32 and tag == 'f64':
                continue                                 # (its values are not float32 numbers)
            M = dense(kind, type, norm, direction, x.shape[-1])
            got = host(L, kind, rk[0], rk[1], 0, x, 1, dtype)
            b = R.bound(M, x, dtype) + FIXTURE_TOL * np.abs(x).sum(-1, keepdims=True)
            assert R.ratio(got, fx[f'y_{kind}_{type}_{norm}_{direction}_{tag}'], b) <= 1, (kind, type, norm, direction)
        for N in (1, 5, 9, 17):
            key = f'mat_{kind}_{type}_{norm}_{direction}_{N}'
            if key in fx:
                eye = np.eye(N, dtype=dtype)
                got = host(L, kind, rk[0], rk[1], 0, eye, 0, dtype)
                b = R.bound(dense(kind, type, norm, direction, N), eye, dtype, axis=0) + FIXTURE_TOL
                assert R.ratio(got, fx[key], b) <= 1, key


def test_host_routine_in_place_and_zeros(L):
    x = np.random.default_rng(3).standard_normal((3, 17, 5))
    want = host(L, 'dst', 3, 'ortho', 0, x, 1, np.float64)
    buf = x.copy()
    rc = L.nfm_rt_transform_host(1, 1, 3, 2, 0, 17, 3, 5, buf.ctypes.data, buf.ctypes.data)
    assert rc == 0 and np.array_equal(buf, want)
    z = host(L, 'dct', 2, 'ortho', 0, np.zeros((4, 9)), 1, np.float32)
    assert np.all(z == 0)


def public(kind, direction):
    from nitorch_fastmath_amd import realtransforms as RT
    name = ('i' if direction == 'inv' else '') + kind
    return getattr(RT, name), getattr(RT, name + 'n')


def test_torch_composition_reproduces_the_fixture_on_cpu(fx):
    for kind, type, norm, direction in cases():
        fn, fnn = public(kind, direction)
        key = f'{kind}_{type}_{norm}_{direction}'
        for tag, dtype in (('f32', np.float32), ('f64', np.float64)):
            x = fx[f'x_{tag}']
            got = fn(torch.from_numpy(x.astype(dtype)), -1, norm, type)
            assert got.dtype == (torch.float32 if dtype == np.float32 else torch.float64) and not got.is_cuda
            M = dense(kind, type, norm, direction, x.shape[-1])
            b = R.bound(M, x, dtype) + FIXTURE_TOL * np.abs(x).sum(-1, keepdims=True)
            assert R.ratio(got.numpy(), fx[f'y_{key}_{tag}'], b) <= 1, (key, tag)
        for N in fx['ns']:
            if f'mat_{key}_{N}' in fx:               # unit impulses, float64: FFT-sized errors (module docstring)
                got = fn(torch.eye(int(N), dtype=torch.float64), 0, norm, type).numpy()
                assert np.abs(got - fx[f'mat_{key}_{N}']).max() <= FIXTURE_TOL, (key, N)
        xnd = torch.from_numpy(fx['x_nd'])
        for case, dim in (('02', [0, 2]), ('all', None)):
            got = fnn(xnd, dim, norm, type).numpy()
            want = fx[f'nd_{key}_{case}']
            assert np.abs(got - want).max() <= FIXTURE_TOL * np.abs(fx['x_nd']).sum(), (key, case)


def test_torch_composition_at_257():
    """the length just past the largest cap a build may have, every kind, type and norm, dense random lines"""
    rng = np.random.default_rng(11)
    for dtype, tdtype in ((np.float32, torch.float32), (np.float64, torch.float64)):
        x = rng.standard_normal((3, 257)).astype(dtype)
        for kind, type, norm, direction in cases():
            fn, _ = public(kind, direction)
            M = dense(kind, type, norm, direction, 257)
            got = fn(torch.from_numpy(x), -1, norm, type)
            assert got.dtype == tdtype
            r = R.ratio(got.numpy(), R.apply(M, x), R.bound(M, x, dtype))
            assert r <= 1, (kind, type, norm, direction, dtype, r)


def test_argument_rules_on_cpu():
    from nitorch_fastmath_amd import realtransforms as RT
    x = torch.randn(4, 6, dtype=torch.float64)
    assert torch.equal(RT.dct(x, None), RT.dct(x, -1)) and torch.equal(RT.dct(x, norm=None), RT.dct(x))
    assert torch.allclose(RT.dctn(x), RT.dct(RT.dct(x, 0), 1)) and torch.equal(RT.dctn(x, [-1]), RT.dct(x, -1))
    assert torch.equal(RT.dst(x, type=1, norm='ortho_scipy'), RT.dst(x, type=1, norm='ortho'))
    assert torch.allclose(RT.idct(RT.dct(x, 0, 'forward', 3), 0, 'forward', 3), x)
    for bad in (0, 4, '2'):
        with pytest.raises(ValueError):
            RT.dct(x, type=bad)
        with pytest.raises(ValueError):
            RT.idstn(x, type=bad)
    with pytest.raises(ValueError):
        RT.dct(torch.ones(3, 1), -1, type=1)
    with pytest.raises(ValueError):
        RT.dct(x, norm='orthogonal')
    with pytest.raises(IndexError):
        RT.dct(x, 2)
    assert RT.dct(torch.ones(3, 4, dtype=torch.float16)).dtype == torch.float32
    assert RT.dst(torch.ones(3, 4, dtype=torch.int32)).dtype == torch.float64
    assert RT.dctn(torch.zeros(0, 4)).shape == (0, 4)
    xt = x.t()
    assert torch.allclose(RT.dst(xt, 0, 'ortho', 3), RT.dst(xt.contiguous(), 0, 'ortho', 3))
    assert torch.allclose(RT.dct(x[:, ::2], 1), RT.dct(x[:, ::2].contiguous(), 1))


def test_gradcheck_on_cpu():
    from nitorch_fastmath_amd import realtransforms as RT
    x = torch.randn(3, 5, 4, dtype=torch.float64, requires_grad=True)
    for kind in R.KINDS:
        for type in R.TYPES:
            for norm in R.NORMS:
                fn = getattr(RT, kind)
                assert torch.autograd.gradcheck(lambda t: fn(t, 1, norm, type), (x,))
    assert torch.autograd.gradcheck(lambda t: RT.idstn(t, [0, 2], 'ortho_scipy', 3), (x,))
    assert torch.autograd.gradgradcheck(lambda t: RT.dctn(t, None, 'ortho', 1), (x,))
