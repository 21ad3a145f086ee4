"""CPU-side checks of `sym.sym_funm` (spectral functions of compact symmetric matrices): the C ABI's answers
without a GPU, the compiled caps and the code-object census, the scalar pieces (`nfm_sym_funm_host_eval`: the source
the kernels run) against mpmath, the reference model of tests/_symfun_ref.py, the torch route `_symfun` on CPU
tensors, and the facade's argument errors."""
import ctypes
import glob
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _symfun_ref as R

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
FLOOR = {('f32', 0): 8, ('f64', 0): 6, ('f32', 1): 6, ('f64', 1): 4}       # the required orders
DT = {'f32': 0, 'f64': 1}


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_bound(L):
    from nitorch_fastmath_amd import _lib
    for name in ('nfm_sym_funm', 'nfm_sym_funm_backward', 'nfm_sym_funm_max_order', 'nfm_sym_funm_host_eval'):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name]
    assert _lib.FUN == {'exp': 0, 'log': 1, 'sqrt': 2, 'rsqrt': 3, 'pow': 4, 'clamp': 5}
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for k, v in _lib.FUN.items():
        assert f'#define NFM_FUN_{k.upper()} {v}\n' in hdr


def test_caps_meet_the_floor(L):
    for (dn, bwd), floor in FLOOR.items():
        cap = L.nfm_sym_funm_max_order(DT[dn], bwd)
        assert floor <= cap <= 8, (dn, bwd, cap)
    assert L.nfm_sym_funm_max_order(7, 0) == 0 and L.nfm_sym_funm_max_order(-1, 1) == 0


def _call(L, bwd, dtype=0, M=3, fn=1, p=0.0, has_min=0, vmin=0.0, no=1, ni=1, ops=None, ptr=4096):
    from nitorch_fastmath_amd import _lib
    n_op = 3 if bwd else 2
    ops = [_lib.Operand(ptr, 0, 1, 0, 1) for _ in range(n_op)] if ops is None else ops
    refs = [None if o is None else ctypes.byref(o) for o in ops]
    f = L.nfm_sym_funm_backward if bwd else L.nfm_sym_funm
    return f(dtype, M, fn, p, has_min, vmin, no, ni, *refs, None)


@pytest.mark.parametrize('bwd', [0, 1])
def test_argument_errors_without_a_gpu(L, bwd):
    """the canonical bad calls of tests/test_abi_sweep_host.py, the codes and the precedence of nfm_sym_det, then
    the entry's own checks; every call is refused (or is an empty batch) before any launch"""
    from nitorch_fastmath_amd import _lib
    n_op = 3 if bwd else 2
    good = lambda: _lib.Operand(4096, 0, 1, 0, 1)                      # noqa: E731
    assert _call(L, bwd, dtype=7) == EDTYPE
    assert _call(L, bwd, ni=-1) == EINVAL
    assert _call(L, bwd, no=65536) == ESIZE
    assert _call(L, bwd, M=0) == ESIZE and _call(L, bwd, M=17) == ESIZE
    for k in range(n_op):
        with_k = lambda o: [o if i == k else good() for i in range(n_op)]          # noqa: E731
        assert _call(L, bwd, ops=with_k(None)) == EINVAL
        assert _call(L, bwd, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
        assert _call(L, bwd, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    assert _call(L, bwd, dtype=7, M=17) == EDTYPE
    assert _call(L, bwd, M=17, ops=[None] + [good() for _ in range(n_op - 1)]) == ESIZE
    assert _call(L, bwd, dtype=7, ops=[None] + [good() for _ in range(n_op - 1)]) == EDTYPE
    assert _call(L, bwd, ni=0, ptr=None) == OK
    # own checks: the function code, the cap, p and vmin finite, clamp needs has_min
    assert _call(L, bwd, fn=6) == EINVAL and _call(L, bwd, fn=-1) == EINVAL
    for dn in ('f32', 'f64'):
        cap = L.nfm_sym_funm_max_order(DT[dn], bwd)
        assert _call(L, bwd, dtype=DT[dn], M=cap, ni=0) == OK
        assert _call(L, bwd, dtype=DT[dn], M=cap + 1, ni=0) == ESIZE
    assert _call(L, bwd, fn=4, p=float('nan')) == EINVAL and _call(L, bwd, fn=4, p=float('inf')) == EINVAL
    assert _call(L, bwd, has_min=1, vmin=float('nan')) == EINVAL
    assert _call(L, bwd, fn=5, has_min=0) == EINVAL
    assert _call(L, bwd, fn=5, has_min=1, vmin=0.5, ni=0) == OK
    assert _call(L, bwd, fn=9, M=9) == EINVAL          # the function code before the cap


def test_host_eval_argument_errors(L):
    x = np.ones(2)
    p = x.ctypes.data
    assert L.nfm_sym_funm_host_eval(7, 0, 0.0, 0, 0.0, 2, p, p, p) == EDTYPE
    assert L.nfm_sym_funm_host_eval(1, 6, 0.0, 0, 0.0, 2, p, p, p) == EINVAL
    assert L.nfm_sym_funm_host_eval(1, 5, 0.0, 0, 0.0, 2, p, p, p) == EINVAL
    assert L.nfm_sym_funm_host_eval(1, 0, 0.0, 0, 0.0, -1, p, p, p) == EINVAL
    assert L.nfm_sym_funm_host_eval(1, 0, 0.0, 0, 0.0, 2, None, p, p) == EINVAL
    assert L.nfm_sym_funm_host_eval(1, 0, 0.0, 0, 0.0, 0, None, None, None) == OK


# ------------------------------------------------------------------------------------------------ the census
def _census():
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_symfun_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_symfun_kernels_in_the_census(L):
    """every (dtype, N <= cap, direction) is compiled, none beyond the cap, none with a private segment"""
    rows = _census()
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    names = [k['kernel'] for k in rows]
    for dn, t in (('f32', 'float'), ('f64', 'double')):
        for bwd, op in ((0, 'SymFunOp'), (1, 'SymFunBwdOp')):
            cap = L.nfm_sym_funm_max_order(DT[dn], bwd)
            for N in range(1, 10):
                have = any(f'{op}<{t}, {N}>' in n for n in names)
                assert have == (N <= cap), (dn, op, N, cap)


# ------------------------------------------------------------------------------------------------ scalar pieces
def _host_eval(L, dn, fn, p, vmin, lam):
    from nitorch_fastmath_amd import _lib
    lam = np.ascontiguousarray(lam, R.NP[dn])
    n = len(lam)
    f, dd = np.empty(n, lam.dtype), np.empty((n, n), lam.dtype)
    rc = L.nfm_sym_funm_host_eval(DT[dn], _lib.FUN[fn], 0.0 if p is None else p, int(vmin is not None),
                                  0.0 if vmin is None else vmin, n, lam.ctypes.data, f.ctypes.data, dd.ctypes.data)
    assert rc == 0
    return f, dd


def _mp_f(mp, fn, p, x):
    return {'exp': mp.exp, 'log': mp.log, 'sqrt': mp.sqrt, 'rsqrt': lambda v: 1 / mp.sqrt(v),
            'pow': lambda v: mp.power(v, mp.mpf(p)), 'clamp': lambda v: v}[fn](x)


def _mp_fprime(mp, fn, p, x):
    return {'exp': mp.exp, 'log': lambda v: 1 / v, 'sqrt': lambda v: 1 / (2 * mp.sqrt(v)),
            'rsqrt': lambda v: -1 / (2 * v * mp.sqrt(v)), 'pow': lambda v: mp.mpf(p) * mp.power(v, mp.mpf(p) - 1),
            'clamp': lambda v: mp.mpf(1)}[fn](x)


def _pairs(dn, fn, vmin, rng):
    """(a, b) of the dtype: a = b; a = b (1 + 2^-k u) for every k up to the mantissa length (exp: a = b + 40 2^-k u);
    ratios up to e^6; with a clamp, pairs on both sides of it and both below it"""
    T = R.NP[dn]
    mant = 24 if dn == 'f32' else 53
    bases = (-30.0, -1.0, 0.5, 20.0) if fn == 'exp' else (0.3, 1.0, 7.5)
    out = []
    for b in bases:
        b = T(b * rng.uniform(0.9, 1.1))
        out.append((b, b))
        for k in range(mant + 1):
            u = rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0])
            a = T(b + 40.0 * 2.0 ** -k * u) if fn == 'exp' else T(b * (1 + 2.0 ** -k * (u if k else abs(u))))
            if fn == 'exp' and a > 40:
                a = T(b - 40.0 * 2.0 ** -k * abs(u))
            out.append((a, b))
        if fn != 'exp':
            for r in (0.3, 1.0, 2.5, 6.0):
                out.append((T(b * np.exp(r)), b))
                out.append((b, T(b * np.exp(r))))
    if vmin is not None:
        m = T(vmin)
        for d1, d2 in ((0.5, 0.25), (0.5, 1e-3), (1e-4, 0.3), (0.7, 0.7)):
            out += [(T(m + d1), T(m - d2)), (T(m - d2), T(m + d1))]          # both sides
        out += [(T(m - 0.3), T(m - 0.1)), (T(m - 0.2), T(m - 0.2)), (m, m), (T(m + 0.5), T(m + 0.5))]   # below; equal
    return out


@pytest.mark.parametrize('fn,with_min', [(f, m) for f in R.FUNCS for m in (False, True) if m or f != 'clamp'])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_scalar_pieces_against_mpmath(L, dn, fn, with_min):
    """f and f[a, b] of nfm_symfun_ops.hpp: relative error <= 16 eps (exp: (16 + |a| + |b|) eps)"""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    rng = np.random.default_rng(11)
    p = R.POW_P if fn == 'pow' else None
    vmin = (0.6 if fn != 'exp' else -1.5) if with_min else None
    eps = R.eps_of(dn)
    worst_f = worst_d = 0.0
    for a, b in _pairs(dn, fn, vmin, rng):
        f, dd = _host_eval(L, dn, fn, p, vmin, [a, b])
        ma, mb = mp.mpf(float(a)), mp.mpf(float(b))
        vm = None if vmin is None else mp.mpf(float(R.NP[dn](vmin)))       # the clamp is rounded to the dtype
        ca, cb = (ma, mb) if vmin is None else (max(ma, vm), max(mb, vm))
        bar = 16 + (abs(float(ca)) + abs(float(cb)) if fn == 'exp' else 0)
        for got, x, c in ((f[0], ma, ca), (f[1], mb, cb)):
            want = _mp_f(mp, fn, p, c)
            err = abs(mp.mpf(float(got)) - want) / abs(want) if want != 0 else abs(mp.mpf(float(got)))
            worst_f = max(worst_f, float(err) / eps / bar * 16)
            assert err <= bar * eps, (fn, dn, 'f', float(x), float(got), float(want))
        if ma == mb:
            want = _mp_fprime(mp, fn, p, ca) * (1 if (vmin is None or ma >= vm) else 0)
        else:
            want = (_mp_f(mp, fn, p, ca) - _mp_f(mp, fn, p, cb)) / (ma - mb)
        for got in (dd[0, 1], dd[1, 0]):
            err = abs(mp.mpf(float(got)) - want) / abs(want) if want != 0 else abs(mp.mpf(float(got)))
            worst_d = max(worst_d, float(err) / eps / bar * 16)
            assert err <= bar * eps, (fn, dn, 'dd', float(a), float(b), float(got), float(want))
        assert dd[0, 0] == dd[0, 0] and dd[1, 1] == dd[1, 1]
    print(f'{fn} {dn} min={vmin}: worst f {worst_f:.2f}, worst f[a,b] {worst_d:.2f} (of 16)')


def test_host_eval_marks_the_domain(L):
    for fn, lam, bad in (('log', [1.0, 0.0, -1.0], [0, 1, 1]), ('sqrt', [1.0, 0.0, -1.0], [0, 0, 1]),
                         ('rsqrt', [1.0, 0.0, -1.0], [0, 1, 1]), ('pow', [1.0, 0.0, -1.0], [0, 0, 1]),
                         ('exp', [1.0, float('nan'), -1.0], [0, 1, 0])):
        f, dd = _host_eval(L, 'f64', fn, 1.7 if fn == 'pow' else None, None, lam)
        assert list(np.isnan(f).astype(int)) == bad, fn
        assert np.array_equal(np.isnan(dd), np.logical_or.outer(np.array(bad, bool), np.array(bad, bool))), fn
    f, dd = _host_eval(L, 'f64', 'pow', -0.5, None, [1.0, 0.0])
    assert np.isnan(f[1])
    f, dd = _host_eval(L, 'f64', 'log', None, 1e-3, [1.0, -2.0])           # the clamp first, then the domain
    assert np.isfinite(f).all() and abs(f[1] - np.log(1e-3)) <= 1e-15 and dd[1, 1] == 0.0


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize('n', [3, 8])
def test_longdouble_jacobi_agrees_with_mpmath(n):
    mp = pytest.importorskip('mpmath')
    assert R.high_ok(), 'numpy.longdouble has no 64-bit mantissa on this machine'
    mp.mp.dps = 40
    comp, _ = R.batch('f64', n, 'log', nb=8 * 7)
    full = R.unpack(np.asarray(comp[::7]), n)                   # one record of every family, 8 in all
    lam, v = R.jacobi_eigh(full.astype(np.longdouble))
    for k in range(8):
        E, _ = mp.eigsy(mp.matrix(full[k].tolist()))
        want = np.array(sorted(float(e) for e in E))
        scale = np.abs(want).max()
        assert np.abs(lam[k].astype(np.float64) - want).max() <= 4 * 2.0 ** -52 * scale
        resid = full[k].astype(np.longdouble) @ v[k] - v[k] * lam[k][None, :]
        assert np.abs(resid).max() <= 64 * n * float(np.finfo(np.longdouble).eps) * scale
        assert np.abs(v[k].T @ v[k] - np.eye(n)).max() <= 64 * n * float(np.finfo(np.longdouble).eps)


# ------------------------------------------------------------------------------------------------ the torch route
NB_HOST = 7 * 16


def _fallback(comp, fn, p, vmin, g=None):
    from nitorch_fastmath_amd import _symfun
    x = torch.from_numpy(np.array(comp)).requires_grad_(g is not None)
    y = _symfun.sym_funm(x, R.FUNCS.index(fn), p, vmin)
    if g is None:
        return y.detach().numpy(), None
    y.backward(torch.from_numpy(np.array(g)))
    return y.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('fn', R.FUNCS)
@pytest.mark.parametrize('n', [3, 9])
def test_fallback_meets_the_bounds_on_cpu(n, fn):
    """forward and gradient of `_symfun` on CPU tensors, float64, every family (isotropic and repeated included:
    the gradient is finite and within the bound there)"""
    assert R.high_ok()
    comp, cells = R.batch('f64', n, fn, nb=NB_HOST)
    g = R.cotangent('f64', n, nb=NB_HOST)
    p, vmin = R.fn_args(fn)
    mod = R.model('f64', fn, comp, p, vmin, g)
    y, gx = _fallback(comp, fn, p, vmin, g)
    assert np.isfinite(y).all() and np.isfinite(gx).all()
    rf, rb = R.forward_ratio('f64', fn, mod, y), R.backward_ratio('f64', fn, mod, g, gx)
    for fam, sl in cells.items():
        print(f'{fn} n={n} {fam}: forward {rf[sl].max():.2f} backward {rb[sl].max():.2f} (of {R.C})')
    assert rf.max() <= R.C and rb.max() <= R.C, (rf.max(), rb.max())


@pytest.mark.parametrize('fn', R.FUNCS)
def test_fallback_gradcheck(fn):
    from nitorch_fastmath_amd import _symfun
    comp, _ = R.batch('f64', 3, fn, nb=7 * 4)
    x = torch.from_numpy(np.array(comp[:4])).requires_grad_(True)              # 4 `normal` records
    p, vmin = R.fn_args(fn)
    assert torch.autograd.gradcheck(lambda t: _symfun.sym_funm(t, R.FUNCS.index(fn), p, vmin), (x,), eps=1e-6,
                                    atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize('fn', ['log', 'sqrt', 'rsqrt', 'pow'])
def test_fallback_domain_gives_nan_records(fn):
    comp = np.array(R.batch('f64', 3, fn, nb=7 * 4)[0][:5])
    comp[1] = R.pack(np.diag([1.0, -0.5, 2.0])[None])[0]
    comp[3, 4] = np.nan
    p, vmin = R.fn_args(fn)
    g = R.cotangent('f64', 3, nb=5)
    y, gx = _fallback(comp, fn, p, vmin, g)
    for r in (y, gx):
        assert np.isnan(r[[1, 3]]).all() and np.isfinite(r[[0, 2, 4]]).all()
    good, ggood = _fallback(comp[[0, 2, 4]], fn, p, vmin, g[[0, 2, 4]])
    assert np.array_equal(y[[0, 2, 4]], good) and np.array_equal(gx[[0, 2, 4]], ggood)
    y, gx = _fallback(comp, fn, p, 1e-3, g)
    assert np.isnan(y[3]).all() and np.isnan(gx[3]).all() and np.isfinite(y[[0, 1, 2, 4]]).all()
    assert np.isfinite(gx[[0, 1, 2, 4]]).all()


# ------------------------------------------------------------------------------------------------ the facade
def test_facade_rejects_bad_arguments():
    import nitorch_fastmath_amd as N
    from nitorch_fastmath_amd import sym as S
    for name in ('sym_funm', 'sym_expm', 'sym_logm', 'sym_sqrtm', 'sym_rsqrtm', 'sym_powm', 'sym_clampm'):
        assert name in S.__all__ and getattr(N, name) is getattr(S, name)
    x = torch.ones(4, 6)
    with pytest.raises(ValueError, match='min'):
        S.sym_funm(x, 'clamp')
    with pytest.raises(ValueError, match='exponent'):
        S.sym_funm(x, 'pow')
    with pytest.raises(ValueError, match='fn must be'):
        S.sym_funm(x, 'cos')
    with pytest.raises(ValueError, match='not M\\*\\(M\\+1\\)/2'):
        S.sym_funm(torch.ones(4, 5), 'exp')
    with pytest.raises(RuntimeError, match='out='):
        S.sym_funm(x.clone().requires_grad_(True), 'exp', out=torch.empty(4, 6))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.sym_logm(x)
