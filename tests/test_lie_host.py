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


# ------------------------------------------------------------------------------------------ Frechet derivatives:
# the fixture, the float64 truth and the model of tests/_lie_ref.py, before a GPU sees their bounds
def test_frechet_fixture_shapes_and_classes():
    import _lie_ref as R
    g = R.fixture()
    per_order = sum(R.FIXTURE_COUNT[c[0]] for c in R.CLASSES)
    assert per_order == 96 and R.fixture_classes()[-1][1].stop == 96
    for D in R.FIXTURE_ORDERS:
        for k in ('x', 'a', 'b', 'L', 'L2'):
            assert g[f'{k}_{D}'].shape == (96, D, D) and g[f'{k}_{D}'].dtype == np.float64
            assert np.isfinite(g[f'{k}_{D}']).all()
        x = g[f'x_{D}']
        n1 = np.abs(x).sum(1).max(1)
        for cls, sl in R.fixture_classes():
            assert np.allclose(n1[sl], cls[1], rtol=1e-12), (D, cls)
            if cls[0] == 'skew':
                assert np.array_equal(x[sl], -x[sl].transpose(0, 2, 1))
            if cls[0] == 'nilp':
                assert not np.tril(x[sl]).any()


def test_frechet_truth64_agrees_with_the_40_digit_fixture():
    """licenses the float64 block identities as the truth of float32 results: 1e-13 (1 + ||X||_1) relative"""
    import _lie_ref as R
    for D in R.FIXTURE_ORDERS:
        x, a, b, L, L2 = R.fixture_records(D)
        for T, bb in ((L, None), (L2, b)):
            e = R.err(R.frechet_truth64(x, a, bb), T) / (1 + R.norm1(x))
            assert float(e.max()) <= 1e-13, (D, bb is None, float(e.max()))
            assert R.fixture_c_ref(D, 1 if bb is None else 2)
    # the series of a nilpotent matrix ends: the finite sum is the same truth
    x, a, b, L, L2 = R.fixture_records(4)
    sl = slice(78, 96)
    assert float(R.err(R.series_frechet(x[sl], a[sl]), L[sl]).max()) <= 1e-14
    assert float(R.err(R.series_frechet(x[sl], a[sl], b[sl]), L2[sl]).max()) <= 1e-14


N_ACC = 2000           # the draw of test_gpu_lie_derivatives.py (3a)
N_MODEL = 500          # the first records of every class of that same draw: X, A and B are the GPU tests' own


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_frechet_model_meets_the_float32_bounds(D, depth):
    """the bars of test_gpu_lie_derivatives.py (3a) are attainable by the kernel's formulas in float32"""
    import _lie_ref as R
    x, a, b, where = R.all_inputs(N_ACC, D, 'f32', first=N_MODEL)
    b = b if depth == 2 else None
    R.class_verdicts(R.frechet_model(x, a, b, torch.float32), R.frechet_truth64(x, a, b),
                     R.frechet_ref(x, a, b, torch.float32), x, torch.float32, where, f'model float32 D={D} L{depth}')


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('D', [2, 3, 4])
def test_frechet_model_meets_the_float64_bounds(D, depth):
    import _lie_ref as R
    x, a, b, L, L2 = R.fixture_records(D)
    bb = b if depth == 2 else None
    R.class_verdicts(R.frechet_model(x, a, bb, torch.float64), L2 if depth == 2 else L, R.frechet_truth64(x, a, bb),
                     x, torch.float64, R.fixture_classes(), f'model float64 fixture D={D} L{depth}')
    x, a, b, where = R.all_inputs(N_ACC, D, 'f64', first=N_MODEL)
    bb = b if depth == 2 else None
    c = R.c_of(R.frechet_model(x, a, bb, torch.float64), R.frechet_truth64(x, a, bb), x, torch.float64)
    for cls, sl in where:
        msg = R.verdict(c[sl], 2 * R.c_bound(R.fixture_c_ref(D, depth)[cls], D), f'model float64 D={D} L{depth} {cls}')
        assert msg is None, msg


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_frechet_model_closed_forms_and_truncation(dn, D):
    """3b and 3f on the model: X = 0, X = c I, a nilpotent X, and a truncated series in the dtype against the same
    series in float64"""
    import _lie_ref as R
    dtype = R.DT[dn]
    x, a, b = R.inputs(('gen', 2.0), 300, D, dn)
    ad, bd = a.double(), b.double()
    sym = (ad @ bd + bd @ ad) / 2
    z = torch.zeros_like(x)
    assert torch.equal(R.frechet_model(z, a, None, dtype), a)
    R.held(R.frechet_model(z, a, b, dtype), sym, z, dtype, R.C_FLOOR, 'model L2 at X = 0')
    for c in (-3.0, 0.5, 6.0):
        xi = (c * torch.eye(D, dtype=dtype)).expand(300, D, D)
        ec = float(np.exp(c))
        R.held(R.frechet_model(xi, a, None, dtype), ec * ad, xi, dtype, R.C_FLOOR, f'model L at {c} I')
        R.held(R.frechet_model(xi, a, b, dtype), ec * sym, xi, dtype, R.C_FLOOR, f'model L2 at {c} I')
        R.held(R.frechet_truth64(xi, a, b), ec * sym, xi, torch.float64, R.C_FLOOR, f'identity L2 at {c} I')
    # A = X, and L2 symmetric in its directions (each order against the truth, and against each other)
    ex = torch.linalg.matrix_exp(x.double())
    k = R.frechet_model(x, x, None, dtype)
    R.held(k, x.double() @ ex, x, dtype, R.C_FLOOR, 'model L(X, X) = X expm(X)')
    R.held(k, ex @ x.double(), x, dtype, R.C_FLOOR, 'model L(X, X) = expm(X) X')
    t2 = R.frechet_truth64(x, a, b) if D > 1 else torch.exp(x.double()) * ad * bd
    kab, kba = R.frechet_model(x, a, b, dtype), R.frechet_model(x, b, a, dtype)
    c2 = R.C_FLOOR if dn == 'f32' else 2 * R.C_FLOOR          # float64: the truth is of the same precision
    R.held(kab, t2, x, dtype, c2, 'model L2(X, A, B)')
    R.held(kba, t2, x, dtype, c2, 'model L2(X, B, A)')
    R.held(kab, kba.double(), x, dtype, 2 * c2, 'model L2 symmetric')
    for e in (-20, 7):
        assert torch.equal(R.frechet_model(x, a * 2.0 ** e, None, dtype), R.frechet_model(x, a, None, dtype) * 2.0 ** e)
    if D == 1:
        return                       # no nilpotent scalar; order 1 is a closed form that ignores max_order / tol
    xn, an, bn = R.inputs(('nilp', 5.0), 300, D, dn)
    R.held(R.frechet_model(xn, an, bn, dtype), R.series_frechet(xn, an, bn), xn, dtype, R.C_FLOOR, 'model nilpotent')
    for max_order, tol in ((1, 1e-32), (2, 1e-32), (5, 1e-32), (10000, 1e-4), (10000, 1e-12)):
        for cls in (('gen', 0.5), ('gen', 8.0)):
            xc, ac, bc = R.inputs(cls, 300, D, dn)
            for bb in (None, bc):
                k = R.frechet_model(xc, ac, bb, dtype, max_order, tol)
                c = R.truncated_verdict(k, xc, ac, bb, dtype, max_order, tol)
                msg = R.verdict(c, R.C_FLOOR, f'model {dn} D={D} {cls} max_order={max_order} tol={tol:g}')
                assert msg is None, msg


# ------------------------------------------------------------------------------------------ the forward kernels:
# the classes, the conditioning unit and the model of tests/_lie_ref.py, before a GPU sees their bounds
FWD_CASES = [('f32', D) for D in range(1, 9)] + [('f64', D) for D in range(1, 8)]


def test_forward_fixture_is_the_interleaved_float64_draw():
    import _lie_ref as R
    g = R.fwd_fixture()
    n = R.FWD_FIXTURE_COUNT * len(R.FWD_CLASSES_F64)
    assert n == 120
    for D in R.FWD_FIXTURE_ORDERS:
        x, t = R.fwd_fixture_records(D)
        assert x.shape == t.shape == (n, D, D) and x.dtype == t.dtype == torch.float64
        assert torch.equal(x, R.fwd_batch(n, D, 'f64', salt=1)[0])
        assert torch.isfinite(t).all()
    assert g['over_x_4'].shape == g['over_log2_4'].shape == (6, 4, 4)
    assert not ((g['over_log2_4'] > 1022) & (g['over_log2_4'] < 1026)).any() and (g['over_log2_4'].max((1, 2)) > 1026).all()


@pytest.mark.parametrize('dn,D', FWD_CASES)
def test_forward_class_invariants(dn, D):
    """every record of every usable class is finite and inside the range condition (asserted by `fwd_case`); a class
    left out at an order really misses it; the edge records have ||X||_1 a power of two bit for bit, where frexp
    gives f = 0.5 and s = log2 + 1; the structured classes have their structure"""
    import _lie_ref as R
    dtype = R.DT[dn]
    X, idx, T, cond = R.fwd_case(D, dn)
    classes = R.fwd_classes(dn, D)
    assert torch.isfinite(X).all() and torch.isfinite(T).all() and torch.isfinite(cond).all()
    assert len(set(idx[:len(classes)].tolist())) == len(classes)            # every class in every run of records
    for cls in R.FWD_UNUSABLE.get((dn, D), ()):
        assert cls in (R.FWD_CLASSES_F64 if dn == 'f64' else R.FWD_CLASSES)
        x = R.fwd_inputs(cls, R.FWD_N_CLASS, D, dn)
        assert not bool(R.in_range(R.fwd_truth64(x), dtype).all()), cls
    s, m = R.lie_plan(X)[:2]
    if D > 1:
        assert int(s.min()) == 0 and int(s.max()) == 10 and int(m.min()) == 5 and int(m.max()) >= 18
    for q, cls in enumerate(classes):
        x = X[idx == q]
        if cls[0] == 'edge':
            col = torch.zeros(x.shape[0], D, dtype=dtype)
            for i in range(D):
                col = col + x[:, i, :].abs()
            assert torch.equal(col.amax(-1), torch.full((x.shape[0],), cls[1], dtype=dtype)), cls
            assert torch.equal(R.norm1(x), torch.full((x.shape[0],), cls[1], dtype=torch.float64)), cls
            if D > 1:
                assert bool((s[idx == q] == int(np.log2(cls[1])) + 1).all()), cls
        elif cls[0] == 'skew':
            assert torch.equal(x, -x.mT)
        elif cls[0] == 'nilp':
            assert not bool(torch.tril(x).any())
        elif cls[0] == 'tri':
            assert not bool(torch.tril(x, -1).any())
            d = torch.diagonal(x, dim1=-2, dim2=-1)
            assert bool(((d <= 0) & (d >= -3)).all())
        elif cls[0] == 'shift' and D > 1:
            g = x.double() + cls[1] * torch.eye(D, dtype=torch.float64)
            assert bool((R.norm1(g) <= R.SHIFT_NORM * (1 + 1e-5)).all())
        elif cls[0] == 'gen' and D > 1:
            assert torch.allclose(R.norm1(x), torch.tensor(cls[1], dtype=torch.float64), rtol=1e-6)


def test_cond_exp_on_closed_forms():
    """cond_exp of a normal matrix is ||X||_F ||e^X||_2 / ||e^X||_F: D^-1/2 ||X||_F for a skew-symmetric one,
    |c| for c I; order 1: |x|"""
    import _lie_ref as R
    x = R.fwd_inputs(('skew', 200.0), 20, 4, 'f64')
    c, nrm = R.cond_exp(x)
    assert torch.allclose(c, torch.linalg.matrix_norm(x) / 2.0, rtol=1e-9)
    assert torch.allclose(nrm, torch.full_like(nrm, 2.0), rtol=1e-12)
    ci = -7.5 * torch.eye(3, dtype=torch.float64)[None]
    assert torch.allclose(R.cond_exp(ci)[0], torch.tensor([7.5], dtype=torch.float64), rtol=1e-12)
    assert torch.equal(R.cond_exp(torch.tensor([[[-3.0]], [[80.0]]]))[0], torch.tensor([3.0, 80.0], dtype=torch.float64))
    assert torch.equal(R.fwd_unit(ci, torch.float32), 3 * 2.0 ** -23 * R.cond_exp(ci)[0])
    assert torch.equal(R.fwd_unit(ci * 0, torch.float32), torch.tensor([3 * 2.0 ** -23], dtype=torch.float64))


@pytest.mark.parametrize('D', range(2, 8))            # _lie_ref.FWD_FIXTURE_ORDERS
def test_matrix_exp_float64_is_a_good_float32_truth(D):
    """licenses matrix_exp in float64 as the truth of float32 results: on every fixture record its error against the
    40-digit value is within 2^-10 eps(float32) / eps(float64) of the float64 unit, that is 2^-10 of the float32 one"""
    import _lie_ref as R
    assert D in R.FWD_FIXTURE_ORDERS
    x, idx, t, cond = R.fwd_case(D, 'f64')
    c = R.fwd_c(R.fwd_truth64(x), t, x, torch.float64, cond)
    cmax = 2.0 ** -10 * torch.finfo(torch.float32).eps / torch.finfo(torch.float64).eps
    R.fwd_verdicts(c, idx, R.fwd_classes('f64', D), cmax, f'matrix_exp float64 D={D}')


@pytest.mark.parametrize('dn,D', [c for c in FWD_CASES if c[1] > 1])
def test_expm_model_meets_half_the_forward_bound(dn, D):
    """the bar of test_gpu_lie_forward.py is attainable: the kernel's formulas in the dtype stay within C_EXPM / 2
    units of D eps max(1, cond_exp) on the records the GPU test judges (float32 against matrix_exp in float64, float64
    against the 40-digit fixture); the factor 2 is the room a kernel gets for its different fma order"""
    import _lie_ref as R
    from test_gpu_lie import C_EXPM
    x, idx, t, cond = R.fwd_case(D, dn)
    c = R.fwd_c(R.expm_model(x, R.DT[dn])[0], t, x, R.DT[dn], cond)
    R.fwd_verdicts(c, idx, R.fwd_classes(dn, D), C_EXPM / 2, f'model {dn} D={D}')


@pytest.mark.parametrize('D', [2, 3])
def test_expm_model_meets_half_the_forward_bound_on_2000_records(D):
    """the same at 2000 records of every class, where the host can afford them (orders 2, 3: 36000 records, a
    second); every one of them inside the range condition"""
    import _lie_ref as R
    from test_gpu_lie import C_EXPM
    classes = R.fwd_classes('f32', D)
    x = torch.cat([R.fwd_inputs(cls, R.FWD_N_CLASS, D, 'f32') for cls in classes])
    idx = torch.arange(len(classes)).repeat_interleave(R.FWD_N_CLASS)
    t = R.fwd_truth64(x)
    assert bool(R.in_range(t, torch.float32).all())
    c = R.fwd_c(R.expm_model(x, torch.float32)[0], t, x, torch.float32)
    R.fwd_verdicts(c, idx, classes, C_EXPM / 2, f'model f32 D={D}, 2000 records')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('D', [2, 4])
def test_expm_model_is_the_e_of_frechet_model(dn, D):
    """one transcription: with (s, m) pinned, `expm_model` has the bits of the exponential that `frechet_model`
    carries through the same recurrences, at full and at truncated degrees"""
    import _lie_ref as R
    dtype = R.DT[dn]
    for cls in (('gen', 0.5), ('gen', 30.0), ('nilp', 5.0)):
        x, a, b = R.inputs(cls, 64, D, dn)
        for max_order, tol in ((10000, 1e-32), (1, 1e-32), (5, 1e-32), (10000, 1e-4), (10000, 0.0)):
            e, plan = R.expm_model(x, dtype, max_order, tol)
            s, m = R.lie_plan(x, max_order, tol)[:2]
            assert torch.equal(plan[0], s) and torch.equal(plan[1], m)
            assert int(m.max()) <= max_order
            for bb in (None, b):
                assert torch.equal(R.frechet_model(x, a, bb, dtype, plan=plan, with_e=True)[1], e)
            assert torch.equal(R.expm_model(x, dtype, plan=plan)[0], e)
        assert torch.equal(R.truncated_verdict(R.expm_model(x, torch.float64, plan=R.lie_plan(x, 5, 1e-32)[:2])[0],
                                               x, None, None, dtype, 5, 1e-32), torch.zeros(64, dtype=torch.float64))
