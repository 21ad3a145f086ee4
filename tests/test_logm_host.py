"""CPU-side checks of `logm` (logm / meanm): signatures, the compat import path, the C ABI's argument answers,
the fixture itself, and the code-object facts of the new kernels."""
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
    """`_impl/logm.py:102` and `lie.py:13`: names, order and defaults"""
    import nitorch_fastmath_amd as N
    from nitorch_fastmath_amd.logm import logm, meanm
    assert N.logm.__all__ == ['logm', 'meanm'] and N.logm.logm is logm
    assert list(inspect.signature(logm).parameters) == ['mat']
    s = inspect.signature(meanm).parameters
    assert list(s) == ['mats', 'max_iter', 'tol']
    assert (s['max_iter'].default, s['tol'].default) == (1024, 1e-20)


def test_compat_resolves_logm():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        importlib.import_module('nitorch_fastmath')
        from nitorch_fastmath.logm import logm, meanm
        import nitorch_fastmath.logm as nl
        import nitorch_fastmath_amd as N
        assert logm is N.logm.logm and meanm is N.logm.meanm and nl is N.logm
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)


def test_lie_still_raises_and_names_the_module():
    from nitorch_fastmath_amd import lie
    assert lie.__all__ == ['expm', 'expm_derivatives']
    for name in ('logm', 'meanm'):
        with pytest.raises(AttributeError, match=r'does not provide.*nitorch_fastmath_amd\.logm'):
            getattr(lie, name)


def test_facade_refuses_cpu():
    from nitorch_fastmath_amd.logm import logm, meanm
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        logm(torch.eye(3).expand(2, 3, 3))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        meanm(torch.eye(4).expand(5, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        meanm([torch.eye(4), torch.eye(4)])


def test_abi_answers_without_a_gpu(L):
    """orders without a kernel answer NFM_ESIZE (the facade's torch route), bad arguments NFM_EINVAL / EDTYPE;
    empty batches are a no-op"""
    from nitorch_fastmath_amd import _lib
    from nitorch_fastmath_amd import logm as LM
    op = _lib.Operand(None, 0, 0, 0, 0)
    r = ctypes.byref(op)
    for code, dtype in ((_lib.F32, torch.float32), (_lib.F64, torch.float64)):
        top = LM.FORWARD_MAX[dtype]
        assert top >= (6 if dtype == torch.float32 else 4)             # the floor of the orders
        for D in range(1, 18):
            want = 0 if D <= top else -3
            assert L.nfm_lie_logm(code, D, 0, 0, r, r, None) == want, (dtype, D)
            assert L.nfm_lie_logm_solve(code, D, 0, 0, r, r, r, None) == want, (dtype, D)
            assert L.nfm_lie_logm_frechet(code, D, 0, 0, r, r, r, None) == (0 if D <= LM.FRECHET_MAX else -3)
    assert LM.FRECHET_MAX >= 4
    assert L.nfm_lie_logm(_lib.F32, 0, 0, 0, r, r, None) == -3
    assert L.nfm_lie_logm(7, 3, 0, 0, r, r, None) == -2
    assert L.nfm_lie_logm(_lib.F32, 3, -1, 0, r, r, None) == -1
    assert L.nfm_lie_logm(_lib.F32, 3, 1, 4, r, r, None) == -1             # null pointer, nonempty
    assert L.nfm_lie_logm_solve(_lib.F64, 3, 1, 4, r, r, r, None) == -1
    assert L.nfm_lie_logm_frechet(_lib.F64, 3, 1, 4, r, r, r, None) == -1
    assert L.nfm_lie_logm(_lib.F32, 3, 0, 0, None, r, None) == -1          # null operand
    assert L.nfm_version() == 5


def test_fixture_reference_and_truth_agree():
    """The reference (scipy, Schur form) against the 40-digit truth on every class with a real logarithm.
    Its Schur decomposition is backward stable in A, an error of D eps ||A||, which the logarithm turns into
    D eps kappa_1(A) relative to ||log A|| only when ||log A|| is not small against ||A||: hence the factor
    max(1, ||A||_1 / ||T||_1) (the class ||X||_1 = 1e-3 needs it).  eps is the INPUT's: scipy decomposes a
    float32 matrix in float32 and only the output is float64."""
    g = np.load(os.path.join(GOLDEN, 'logm.npz'))
    worst = 0.0
    for dt, eps in (('f32', 2.0 ** -23), ('f64', 2.0 ** -52)):
        for D in range(1, 9):
            x, ref, true, cls = (g[f'{k}_{dt}_{D}'] for k in ('x', 'ref', 'true', 'cls'))
            assert ref.dtype == np.float64 and np.isfinite(true).all() and len(cls) == len(x)
            assert g[f'bad_{dt}_{D}'].shape == (5, D, D)
            x = x.astype(np.float64)
            err = np.abs(ref - true).max((1, 2)) / np.abs(true).max((1, 2))
            kap = np.linalg.cond(x, 1)
            fac = np.maximum(1, np.abs(x).sum(1).max(1) / np.abs(true).sum(1).max(1))
            worst = max(worst, (err / (D * eps * kap * fac)).max())
    assert worst <= 16, worst
    for name in ('rigid', 'affine'):
        assert np.abs(g[f'{name}_ref'] - g[f'{name}_true']).max() <= 1e-13
    for name, n in (('rigid', 7), ('affine', 12), ('spd', 16)):
        assert g[f'meanm_{name}_x'].shape[0] == n and float(g[f'meanm_{name}_sos']) <= 1e-20


def test_torch_route_on_the_fixture():
    """the torch route is plain torch: on the CPU it meets the float64 fixture, and keeps the NaN policy"""
    from nitorch_fastmath_amd.logm import _logm_torch
    g = np.load(os.path.join(GOLDEN, 'logm.npz'))
    for D in (2, 5, 8):
        x, true = torch.from_numpy(g[f'x_f64_{D}']), torch.from_numpy(g[f'true_f64_{D}'])
        k = _logm_torch(x)
        err = (k - true).abs().amax((1, 2)) / true.abs().amax((1, 2))
        assert bool((err <= 16 * D * 2.0 ** -52 * torch.linalg.cond(x, 1)).all())
        assert torch.isnan(_logm_torch(torch.from_numpy(g[f'bad_f64_{D}']))).all()
    assert torch.equal(_logm_torch(torch.eye(4).expand(3, 4, 4)), torch.zeros(3, 4, 4))


def _hard_cases():
    import _logm_ref as R
    return [(dt, D) for dt in R.ORDERS for D in list(R.ORDERS[dt]) + list(R.ROUTE_ORDERS[dt])]


def test_hard_fixture_invariants():
    """tests/golden/logm_hard.npz: every truth validated at 1e-30, the classes and tiers as the generator states them,
    every class of both tiers at every order with a kernel"""
    import _logm_ref as R
    g = R.load()
    demoted = {tuple(s.split('/')[:3]) for s in g['demoted'].tolist()}
    no_pair = set(g['no_pair'].tolist())
    assert all(s.endswith('/rot') for s in no_pair)
    for dt, D in _hard_cases():
        rec = R.records(g, dt, D)
        route = D in R.ROUTE_ORDERS[dt]
        n = len(rec['x'])
        assert rec['x'].dtype == (np.float32 if dt == 'f32' else np.float64) and rec['true'].dtype == np.float64
        assert rec['x'].shape == rec['true'].shape == (n, D, D)
        assert np.isfinite(rec['x']).all() and np.isfinite(rec['true']).all()
        assert (rec['res'] <= 1e-30).all()
        assert (rec['nK'] > 0).all() and (rec['cl'] > 0).all()
        np.testing.assert_allclose(rec['cl'], rec['nK'] * R.fro(rec['x']) / R.fro(rec['true']), rtol=1e-12)
        want = []
        for cls, (tier, pars) in R.CLASSES.items():
            if route and tier == R.TIER_B:
                continue
            k = 2 if route else R.PER_CLASS
            tier = R.TIER_B if (dt, str(D), cls) in demoted else tier
            name, p = 'rot' if cls == 'rotb' else cls, pars[dt]
            want += [(name, tier, float(p[(i + D) % len(p)])) for i in range(k)]
        assert list(zip(rec['cls'].tolist(), rec['tier'].tolist(), rec['par'].tolist())) == want, (dt, D)
        if D in R.FRECHET_ORDERS:
            assert rec['E'].shape == rec['L'].shape == (n, D, D) and np.isfinite(rec['L']).all()
            # ||L_log(x, E)||_F <= ||K||_2 ||E||_F
            assert (R.fro(rec['L']) <= rec['nK'] * R.fro(rec['E']) * (1 + 1e-6)).all()
        if not route:
            sm, sa, st = (g[f'{k}_{dt}_{D}'] for k in ('sm', 'sa', 'strue'))
            # every tier-A class but those of which the generator found no M^-1 A with a real logarithm
            ta = [c for c, (t, _) in R.CLASSES.items() if t == R.TIER_A and f'{dt}/{D}/{c}' not in no_pair]
            assert g[f'scls_{dt}_{D}'].tolist() == ta and len(ta) >= 4
            assert sm.shape == sa.shape == st.shape == (len(ta), D, D) and (g[f'sres_{dt}_{D}'] <= 1e-30).all()
            np.testing.assert_allclose(g[f'skap_{dt}_{D}'], np.linalg.cond(sm.astype(np.float64), 1), rtol=1e-9)
            assert g[f'skap_{dt}_{D}'].max() <= (1e4 if dt == 'f32' else 1e8) * 10


def test_hard_fixture_truths_validate_again():
    """one record of every class (float64, order 3) through mpmath again: the residual the generator recorded"""
    import mpmath
    import _logm_ref as R
    g = R.load()
    rec = R.records(g, 'f64', 3)
    for i in range(0, len(rec['x']), R.PER_CLASS):
        with mpmath.workdps(60):
            A = R.mp_of(rec['x'][i])
            L, res, _ = R.mp_logm(A)
            assert L is not None and res <= 1e-30
            assert np.abs(R.mp_to_np(L) - rec['true'][i]).max() <= 2.0 ** -50 * np.abs(rec['true'][i]).max()


@pytest.mark.parametrize('dt,D', _hard_cases())
def test_torch_route_on_the_hard_fixture(dt, D):
    """`_logm_torch`, the kernel's algorithm, on the CPU over the whole hard fixture under the bounds the kernels are
    held to (tests/_logm_ref.py): tier A without a NaN, tier B NaN or within eps m^2, the jvp, logm_solve"""
    import _logm_ref as R
    from torch.func import jvp
    from nitorch_fastmath_amd.logm import _logm_torch
    g = R.load()
    rec = R.records(g, dt, D)
    x = torch.from_numpy(rec['x'])
    ok, r, what = R.check_logm(_logm_torch(x).numpy(), rec, dt)
    print(dt, D, 'route worst err / (eps m):', {k: f'{v:.3g}' for k, v in R.worst_by_class(r, rec).items()})
    assert ok.all(), [(rec['cls'][i], float(rec['par'][i]), what[i], float(r[i])) for i in np.flatnonzero(~ok)]
    if D in R.FRECHET_ORDERS:
        l = jvp(_logm_torch, (x,), (torch.from_numpy(rec['E']),))[1].numpy()
        ta = rec['tier'] == R.TIER_A
        rf = R.frechet_ratio(l, rec, dt)
        print(dt, D, 'jvp worst err / (D eps m^2 ||K|| ||E||):',
              {k: f'{v:.3g}' for k, v in R.worst_by_class(rf, rec).items()})
        assert np.isfinite(l[ta]).all() and (rf[ta] <= R.C_LOGM).all(), rf
    if D not in R.ROUTE_ORDERS[dt]:
        sm, sa, st, kap, cl = (g[f'{k}_{dt}_{D}'] for k in ('sm', 'sa', 'strue', 'skap', 'scl'))
        k = _logm_torch(torch.linalg.solve(torch.from_numpy(sm), torch.from_numpy(sa))).double().numpy()
        rs = R.fro(k - st) / R.fro(st) / (D * R.EPS[dt] * kap * R.m_of(cl))
        assert np.isfinite(k).all() and (rs <= R.C_LOGM).all(), rs


def _census():
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_logm.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_logm_kernels_in_the_census():
    """every (op, dtype, order) the dispatch reaches is compiled, without scratch, and none beyond it"""
    from nitorch_fastmath_amd import logm as LM
    rows = _census()
    names = [k['kernel'] for k in rows]
    assert not [k['kernel'] for k in rows if k['scratch']]
    for t, dtype in (('float', torch.float32), ('double', torch.float64)):
        for D in range(1, 10):
            for op in ('LogmOp', 'LogmSolveOp'):
                assert any(f'{op}<{t}, {D}>' in n for n in names) == (D <= LM.FORWARD_MAX[dtype]), (op, t, D)
            assert any(f'LogmFrechetOp<{t}, {D}>' in n for n in names) == (D <= LM.FRECHET_MAX), (t, D)
