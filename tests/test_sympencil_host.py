"""CPU-side checks of the two-matrix spectral functions of `sym` (`sym_pencil_funm`, `sym_geneigvals`, `sym_dist`):
the C ABI's answers without a GPU, the compiled caps and the code-object census, the reference model of
tests/_sympencil_ref.py against mpmath, the composition route `_sympencil` on CPU tensors, and the facade's
argument errors."""
import ctypes
import glob
import os
import re
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _symfun_ref as R
import _sympencil_ref as P

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
DT = {'f32': 0, 'f64': 1}
OPS = {'funm': 0, 'funm_backward': 1, 'eig': 2, 'dist_backward': 3}
FLOOR = {('f32', 0): 8, ('f64', 0): 6, ('f32', 2): 8, ('f64', 2): 6,
         ('f32', 1): 4, ('f64', 1): 3, ('f32', 3): 4, ('f64', 3): 3}
ENTRIES = ('nfm_sym_pencil_funm', 'nfm_sym_pencil_funm_backward', 'nfm_sym_pencil_eig',
           'nfm_sym_pencil_dist_backward')
N_OP = {'funm': 3, 'funm_backward': 4, 'eig': 3, 'dist_backward': 4}


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
    for name in ENTRIES + ('nfm_sym_pencil_max_order',):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name]
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for k, v in (('OP_FUNM', _lib.PENCIL_OP_FUNM), ('OP_FUNM_BACKWARD', _lib.PENCIL_OP_FUNM_BACKWARD),
                 ('OP_EIG', _lib.PENCIL_OP_EIG), ('OP_DIST_BACKWARD', _lib.PENCIL_OP_DIST_BACKWARD),
                 ('EIG', _lib.PENCIL_EIG), ('DIST2', _lib.PENCIL_DIST2), ('DIST', _lib.PENCIL_DIST)):
        assert f'#define NFM_PENCIL_{k} {v}\n' in hdr


def test_header_and_signature_table_agree(L):
    """the number and the kinds of the arguments the header declares are those of the binding"""
    from nitorch_fastmath_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    kinds = {'int': ctypes.c_int, 'double': ctypes.c_double, 'int64_t': ctypes.c_int64}
    for name in ENTRIES + ('nfm_sym_pencil_max_order',):
        m = re.search(r'\bint ' + name + r'\(([^)]*)\);', hdr)
        assert m, name
        args = [' '.join(a.split()) for a in m.group(1).split(',')]
        want = [ctypes.c_void_p if '*' in a else kinds[a.rsplit(' ', 1)[0]] for a in args]
        assert want == _lib.SIGNATURES[name], name
    assert open(os.path.join(ROOT, 'INTEGRATION.md')).read().count('`nfm_sym_pencil_') >= 5


def test_caps_meet_the_floor(L):
    for (dn, op), floor in FLOOR.items():
        cap = L.nfm_sym_pencil_max_order(DT[dn], op)
        assert floor <= cap <= 8, (dn, op, cap)
    assert L.nfm_sym_pencil_max_order(7, 0) == 0 and L.nfm_sym_pencil_max_order(0, 4) == 0
    assert L.nfm_sym_pencil_max_order(1, -1) == 0


def _call(L, op, dtype=0, M=3, fn=1, p=0.0, has_min=0, mode=1, no=1, ni=1, ops=None, ptr=4096):
    from nitorch_fastmath_amd import _lib
    n_op = N_OP[op]
    ops = [_lib.Operand(ptr, 0, 1, 0, 1) for _ in range(n_op)] if ops is None else ops
    refs = [None if o is None else ctypes.byref(o) for o in ops]
    f = getattr(L, 'nfm_sym_pencil_' + op)
    if op.startswith('funm'):
        return f(dtype, M, fn, p, has_min, 0.0, no, ni, *refs, None)
    return f(dtype, M, mode, no, ni, *refs, None)


@pytest.mark.parametrize('op', list(OPS))
def test_argument_errors_without_a_gpu(L, op):
    """the canonical bad calls of tests/test_abi_sweep_host.py with the codes and the precedence of nfm_sym_funm,
    then the entry's own checks; every call is refused (or is an empty batch) before any launch"""
    from nitorch_fastmath_amd import _lib
    n_op = N_OP[op]
    good = lambda: _lib.Operand(4096, 0, 1, 0, 1)                      # noqa: E731
    assert _call(L, op, dtype=7) == EDTYPE
    assert _call(L, op, ni=-1) == EINVAL
    assert _call(L, op, no=65536) == ESIZE
    assert _call(L, op, M=0) == ESIZE and _call(L, op, M=17) == ESIZE
    for k in range(n_op):
        with_k = lambda o: [o if i == k else good() for i in range(n_op)]          # noqa: E731
        assert _call(L, op, ops=with_k(None)) == EINVAL
        assert _call(L, op, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
        assert _call(L, op, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    assert _call(L, op, dtype=7, M=17) == EDTYPE
    assert _call(L, op, M=17, ops=[None] + [good() for _ in range(n_op - 1)]) == ESIZE
    assert _call(L, op, dtype=7, ops=[None] + [good() for _ in range(n_op - 1)]) == EDTYPE
    assert _call(L, op, ni=0, ptr=None) == OK
    for dn in ('f32', 'f64'):
        cap = L.nfm_sym_pencil_max_order(DT[dn], OPS[op])
        assert _call(L, op, dtype=DT[dn], M=cap, ni=0) == OK
        assert _call(L, op, dtype=DT[dn], M=cap + 1, ni=0) == ESIZE
    if op.startswith('funm'):          # the function code (no clamp, no has_min), then the cap, then p finite
        assert _call(L, op, fn=6) == EINVAL and _call(L, op, fn=-1) == EINVAL
        assert _call(L, op, fn=5) == EINVAL and _call(L, op, has_min=1) == EINVAL
        assert _call(L, op, fn=4, p=float('nan')) == EINVAL and _call(L, op, fn=4, p=float('inf')) == EINVAL
        assert _call(L, op, fn=9, M=9) == EINVAL
        assert _call(L, op, fn=4, p=float('nan'), M=9) == ESIZE
        assert _call(L, op, fn=4, p=0.5, ni=0) == OK
    else:                               # the mode, then the cap
        assert _call(L, op, mode=3) == EINVAL and _call(L, op, mode=-1) == EINVAL
        assert _call(L, op, mode=0, ni=0) == (OK if op == 'eig' else EINVAL)
        assert _call(L, op, mode=7, M=9) == EINVAL
        assert _call(L, op, mode=2, ni=0) == OK


# ------------------------------------------------------------------------------------------------ the census
def _census():
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_sympencil_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_sympencil_kernels_in_the_census(L):
    """every (dtype, op, N <= cap) is compiled, none beyond the cap, none with a private segment"""
    rows = _census()
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    names = [k['kernel'] for k in rows]
    ops = ((0, ('PencilFunOp<{t}, {N}>',)), (1, ('PencilFunBwdOp<{t}, {N}>',)),
           (2, ('PencilEigOp<{t}, {N}, false>', 'PencilEigOp<{t}, {N}, true>')), (3, ('PencilDistBwdOp<{t}, {N}>',)))
    for dn, t in (('f32', 'float'), ('f64', 'double')):
        for op, pats in ops:
            cap = L.nfm_sym_pencil_max_order(DT[dn], op)
            for N in range(1, 10):
                for pat in pats:
                    have = any(pat.format(t=t, N=N) in n for n in names)
                    assert have == (N <= cap), (dn, pat, N, cap)


# ------------------------------------------------------------------------------------------------ the model
def test_model_agrees_with_mpmath():
    """one record of every family at n = 3: the generalised eigenvalues (mpmath's eigsy of the whitened matrix built
    from its own Cholesky factor), the function and the distance from them"""
    mp = pytest.importorskip('mpmath')
    assert R.high_ok(), 'numpy.longdouble has no 64-bit mantissa on this machine'
    mp.mp.dps = 40
    n, fn = 3, 'log'
    ca, cb, cells = P.batch('f64', n, fn)
    pick = [sl.start for sl in cells.values()]
    mod = P.model('f64', fn, ca[pick], cb[pick])
    A, B = R.unpack(np.asarray(ca[pick]), n), R.unpack(np.asarray(cb[pick]), n)
    for k in range(len(pick)):
        sc = float(mod['scale'][k])          # the `scaled` pair divided by its power of two (exact)
        Am, Bm = mp.matrix((A[k] / sc).tolist()), mp.matrix((B[k] / sc).tolist())
        Li = mp.inverse(mp.cholesky(Am))
        Cm = Li * Bm * Li.T
        E, Q = mp.eigsy((Cm + Cm.T) / 2)
        order = sorted(range(n), key=lambda i: E[i])
        mu = [E[i] for i in order]
        scale = max(abs(float(m)) for m in mu)
        kap = float(mod['kappa'][k])
        assert max(abs(float(mod['mu'][k][i]) - float(mu[i])) for i in range(n)) <= 64 * 2.0 ** -52 * kap * scale
        d2 = sum(mp.log(m) ** 2 for m in mu)
        assert abs(float(mod['d2'][k]) - float(d2)) <= 64 * 2.0 ** -52 * kap * max(float(d2), 2.0 ** -52) * 4
        # G = A^1/2 log(A^-1/2 B A^-1/2) A^1/2 = L log(L^-1 B L^-T) L^T for any factor A = L L^T
        Lc = mp.cholesky(Am)
        Qm = mp.matrix([[Q[i, j] for j in order] for i in range(n)])
        G = Lc * Qm * mp.diag([mp.log(m) for m in mu]) * Qm.T * Lc.T
        err = max(abs(float(mod['G'][k][i, j] / sc) - float(G[i, j])) for i in range(n) for j in range(n))
        assert err <= 64 * 2.0 ** -52 * kap * float(mod['normA'][k] / sc) * max(float(mod['normF'][k]), 1.0)


def test_constant_follows_the_procedure():
    """C from R_REF; that R_REF still is the composition's worst ratio: test_composition_meets_the_bounds_on_cpu"""
    assert P.C == max(16.0, 2.0 ** np.ceil(np.log2(2 * P.R_REF)))


# ------------------------------------------------------------------------------------------------ the composition route
@pytest.mark.parametrize('fn', P.FUNCS)
@pytest.mark.parametrize('n', [1, 3, 8, 9])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_composition_meets_the_bounds_on_cpu(dn, n, fn):
    """every quantity of `_sympencil` on CPU tensors in the working dtype, every family: within C of the bounds, and
    no worse than the R_REF the constant was derived from"""
    assert R.high_ok()
    _, _, cells = P.batch(dn, n, fn)
    for q, r in P.composition_ratios(dn, n, fn).items():
        assert np.isfinite(r).all(), q
        for fam, sl in cells.items():
            print(f'{dn} n={n} {fn} {q} {fam}: {r[sl].max():.2f} (of {P.C})')
        assert r.max() <= P.C, (q, r.max(), int(r.argmax()))
        assert r.max() <= P.R_REF, (q, r.max(), int(r.argmax()))          # a drift of R_REF would move C


def _pair(n, nb, equal=False):
    ca, cb, cells = P.batch('f64', n, 'log')
    sl = cells['equal' if equal else 'normal']
    return (torch.from_numpy(np.array(ca[sl][:nb])).requires_grad_(True),
            torch.from_numpy(np.array(cb[sl][:nb])).requires_grad_(True))


@pytest.mark.parametrize('fn', P.FUNCS)
def test_composition_gradcheck(fn):
    from nitorch_fastmath_amd import _sympencil
    a, b = _pair(3, 3)
    code = R.FUNCS.index(fn)
    assert torch.autograd.gradcheck(lambda x, y: _sympencil.pencil_funm(x, y, code, P.fn_p(fn)), (a, b), eps=1e-6,
                                    atol=1e-6, rtol=1e-5)


def test_composition_gradcheck_eigenvalues_and_distance():
    from nitorch_fastmath_amd import _sympencil
    a, b = _pair(3, 3)
    assert torch.autograd.gradcheck(_sympencil.geneigvals, (a, b), eps=1e-6, atol=1e-6, rtol=1e-5)
    for squared in (True, False):
        assert torch.autograd.gradcheck(lambda x, y: _sympencil.dist(x, y, squared), (a, b), eps=1e-6, atol=1e-6,
                                        rtol=1e-5)
    a, b = _pair(3, 3, equal=True)          # the isotropic pencil: d2 has a regular minimum there
    assert torch.equal(a, b)
    assert torch.autograd.gradcheck(lambda x, y: _sympencil.dist(x, y, True), (a, b), eps=1e-6, atol=1e-6, rtol=1e-5)
    d2 = _sympencil.dist(a, b, True)
    ga, gb = torch.autograd.grad(d2.sum(), (a, b))
    assert float(ga.abs().max()) <= 1e-13 and float(gb.abs().max()) <= 1e-13
    ga, gb = torch.autograd.grad(_sympencil.dist(a, b, False).sum(), (a, b))
    assert torch.isfinite(ga).all() and torch.isfinite(gb).all()


def test_composition_gives_nan_records():
    from nitorch_fastmath_amd import _sympencil
    ca, cb, _ = P.batch('f64', 3, 'log')
    a, b = np.array(ca[:5]), np.array(cb[:5])
    a[1] = R.pack(np.diag([1.0, -0.5, 2.0])[None])[0]          # a base that is not positive definite
    b[3, 4] = np.nan
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    good = [0, 2, 4]
    for f in (lambda x, y: _sympencil.pencil_funm(x, y, 1), _sympencil.geneigvals, _sympencil.dist):
        r = f(ta, tb).numpy().reshape(5, -1)
        assert np.isnan(r[[1, 3]]).all() and np.isfinite(r[good]).all()
        assert np.array_equal(r[good], f(ta[good], tb[good]).numpy().reshape(3, -1))


# ------------------------------------------------------------------------------------------------ the facade
def test_facade_rejects_bad_arguments():
    import nitorch_fastmath_amd as N
    from nitorch_fastmath_amd import sym as S
    for name in ('sym_pencil_funm', 'sym_geodesic', 'sym_geomean', 'sym_logmap', 'sym_expmap', 'sym_geneigvals',
                 'sym_dist', 'sym_karcher_mean'):
        assert name in S.__all__ and getattr(N, name) is getattr(S, name)
    x = torch.ones(4, 6)
    with pytest.raises(ValueError, match='fn must be'):
        S.sym_pencil_funm(x, x, 'cos')
    with pytest.raises(ValueError, match='fn must be'):
        S.sym_pencil_funm(x, x, 'clamp')
    with pytest.raises(ValueError, match='min / clamp'):
        S.sym_pencil_funm(x, x, 'log', min=0.5)
    with pytest.raises(ValueError, match='min / clamp'):
        S.sym_pencil_funm(x, x, 'log', clamp=0.5)
    with pytest.raises(ValueError, match='exponent'):
        S.sym_pencil_funm(x, x, 'pow')
    with pytest.raises(ValueError, match='not the same order'):
        S.sym_pencil_funm(x, torch.ones(4, 3), 'log')
    with pytest.raises(ValueError, match='not the same order'):
        S.sym_dist(x, torch.ones(4, 10))
    with pytest.raises(ValueError, match='not M\\*\\(M\\+1\\)/2'):
        S.sym_geneigvals(torch.ones(4, 5), torch.ones(4, 5))
    with pytest.raises(RuntimeError, match='out='):
        S.sym_logmap(x.clone().requires_grad_(True), x, out=torch.empty(4, 6))
    with pytest.raises(ValueError, match='batch dimension'):
        S.sym_karcher_mean(x, dim=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.sym_geomean(x, x)
