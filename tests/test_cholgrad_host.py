"""CPU-side checks of the backward kernels of the Cholesky factor (the gradients of sym_chol and sym_chol_apply): the C
ABI's answers without a GPU, the compiled caps and the code-object census, the record routines the kernels run
(`nfm_sym_chol_grad_host`: the same source) and a plain numpy implementation against every bound of
tests/_cholgrad_ref.py, the bad-record rule, the scale equivariance of the factor's gradient, and what the facade and
the torch composition still do on CPU tensors."""
import ctypes
import glob
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _cholgrad_ref as G
import _symchol_ref as C
import _symfun_ref as R

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
FACTOR, APPLY, SCALAR, BACKWARD = range(4)              # NFM_CHOL_CLASS_*
FLOOR = {('f32', FACTOR): 8, ('f64', FACTOR): 6, ('f32', APPLY): 8, ('f64', APPLY): 6}
DT = {'f32': 0, 'f64': 1}
NAMES = ('nfm_sym_chol_grad', 'nfm_sym_chol_grad_max_order', 'nfm_sym_chol_grad_host')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as E
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        E.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_declared_and_bound(L):
    from nitorch_fastmath_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name]
        assert ctypes.POINTER(_lib.Operand) not in _lib.SIGNATURES[name]
        assert f'int {name}(' in hdr
    assert L.nfm_version() == 5


def test_caps_meet_the_floor(L):
    for (dn, cls), floor in FLOOR.items():
        cap = L.nfm_sym_chol_grad_max_order(DT[dn], cls)
        assert floor <= cap <= 8, (dn, cls, cap)
    for dtype, cls in ((7, 0), (-1, 1), (0, SCALAR), (1, BACKWARD), (0, 4), (1, -1)):
        assert L.nfm_sym_chol_grad_max_order(dtype, cls) == 0


# (name, C op code, index of the operand that is not read)
ENTRIES = [('factor', 0, 1), ('factor_factored', 0 | 16, 1), ('apply', 3, None), ('apply_factored', 1 | 16, None)]
N_OP = 4


def _call(L, entry, dtype=0, M=3, op=None, no=1, ni=1, ops=None, ptr=4096):
    from nitorch_fastmath_amd import _lib
    _, code, _ = entry
    ops = [_lib.Operand(ptr, 0, 1, 0, 1) for _ in range(N_OP)] if ops is None else ops
    refs = [None if o is None else ctypes.byref(o) for o in ops]
    return L.nfm_sym_chol_grad(dtype, M, code if op is None else op, no, ni, *refs, None)


@pytest.mark.parametrize('entry', ENTRIES, ids=[e[0] for e in ENTRIES])
def test_argument_errors_without_a_gpu(L, entry):
    """the canonical bad calls of tests/test_symchol_host.py against nfm_sym_chol_grad; every call is refused (or is an
    empty batch) before any launch"""
    from nitorch_fastmath_amd import _lib
    _, code, unread = entry
    good = lambda: _lib.Operand(4096, 0, 1, 0, 1)                      # noqa: E731
    assert _call(L, entry, dtype=7) == EDTYPE
    assert _call(L, entry, ni=-1) == EINVAL
    assert _call(L, entry, no=65536) == ESIZE
    assert _call(L, entry, M=0) == ESIZE and _call(L, entry, M=17) == ESIZE
    for k in range(N_OP):
        with_k = lambda o: [o if i == k else good() for i in range(N_OP)]          # noqa: E731
        if k == unread:            # the factor op has no vector: the argument is not looked at
            assert _call(L, entry, ni=0, ops=with_k(None)) == OK
            assert _call(L, entry, ni=0, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == OK
            continue
        assert _call(L, entry, ops=with_k(None)) == EINVAL
        assert _call(L, entry, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
        assert _call(L, entry, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    assert _call(L, entry, dtype=7, M=17) == EDTYPE
    assert _call(L, entry, M=17, ops=[None] + [good() for _ in range(N_OP - 1)]) == ESIZE
    assert _call(L, entry, dtype=7, ops=[None] + [good() for _ in range(N_OP - 1)]) == EDTYPE
    assert _call(L, entry, ni=0, ptr=None) == OK
    # own checks: the op code (the scalar ops have their own entry), then the cap of the class
    for op in (5, 6, 7, 8, 9, 15, 32, -1, 5 | 16, 6 | 16, 8 | 16, 9 | 16):
        assert _call(L, entry, op=op) == EINVAL, op
    cls = FACTOR if (code & 15) == 0 else APPLY
    for dn in ('f32', 'f64'):
        cap = L.nfm_sym_chol_grad_max_order(DT[dn], cls)
        assert _call(L, entry, dtype=DT[dn], M=cap, ni=0) == OK
        assert _call(L, entry, dtype=DT[dn], M=cap + 1, ni=0) == ESIZE
    assert _call(L, entry, op=9, M=9) == EINVAL          # the op code before the cap
    assert _call(L, entry, op=9, M=17) == ESIZE          # the range of M before the op code


def test_host_entry_argument_errors(L):
    x = np.ones(16)
    p = x.ctypes.data
    H = L.nfm_sym_chol_grad_host
    assert H(7, 2, 0, 1, p, p, p, p) == EDTYPE
    assert H(1, 2, 0, -1, p, p, p, p) == EINVAL
    for op in (5, 6, 7, 8, 9, -1, 32, 5 | 16, 9 | 16):
        assert H(1, 2, op, 1, p, p, p, p) == EINVAL, op
    assert H(1, 0, 0, 1, p, p, p, p) == ESIZE and H(1, 9, 0, 1, p, p, p, p) == ESIZE
    assert H(1, 2, 0, 1, None, p, p, p) == EINVAL and H(1, 2, 0, 1, p, p, None, p) == EINVAL
    assert H(1, 2, 0, 1, p, p, p, None) == EINVAL and H(1, 2, 3, 1, p, None, p, p) == EINVAL
    assert H(1, 2, 0, 0, None, None, None, None) == OK
    assert H(1, 2, 0, 1, p, None, p, p) == OK and H(1, 2, 0 | 16, 1, p, None, p, p) == OK


def test_old_entries_still_refuse_the_factor_and_apply_codes(L):
    from nitorch_fastmath_amd import _lib
    ops = [ctypes.byref(_lib.Operand(4096, 0, 1, 0, 1)) for _ in range(4)]
    p = np.ones(16).ctypes.data
    for op in (0, 1, 2, 3, 4, 3 | 16):
        assert L.nfm_sym_chol_backward(0, 3, op, 1, 1, *ops, None) == EINVAL, op
        assert L.nfm_sym_chol_host(1, 2, op, 1, p, p, p, p) == EINVAL, op
    for cls in (4, 5, -1):
        assert L.nfm_sym_chol_max_order(0, cls) == 0
    assert L.nfm_version() == 5


# ------------------------------------------------------------------------------------------------ the census
def _census():
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_cholgrad_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_cholgrad_kernels_in_the_census(L):
    """every (dtype, class, N <= cap) is compiled, none beyond the cap, none with a private segment"""
    rows = _census()
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    names = [k['kernel'] for k in rows]
    for dn, t in (('f32', 'float'), ('f64', 'double')):
        for cls, pat in ((FACTOR, 'CholFactorGradOp<{t}, {N}>'), (APPLY, 'CholApplyGradOp<{t}, {N}>')):
            cap = L.nfm_sym_chol_grad_max_order(DT[dn], cls)
            for N in range(1, 10):
                have = any(pat.format(t=t, N=N) in n for n in names)
                assert have == (N <= cap), (dn, cls, N, cap)


# ------------------------------------------------------------------------------------------------ the record routines
def host(L, dn, n, op, mat, vec, cot, factored=False):
    """`nfm_sym_chol_grad_host` on contiguous numpy records: the packed gradient (nb, K) or (nb, K + n)"""
    T = R.NP[dn]
    mat = np.ascontiguousarray(mat, T)
    cot = np.ascontiguousarray(cot, T)
    vec = None if op == 'factor' else np.ascontiguousarray(vec, T)
    nb, K = mat.shape
    out = np.full((nb, K if op == 'factor' else K + n), 7.0, T)
    rc = L.nfm_sym_chol_grad_host(DT[dn], n, C.CODE[op] | (C.FACTORED if factored else 0), nb, mat.ctypes.data,
                                  None if vec is None else vec.ctypes.data, cot.ctypes.data, out.ctypes.data)
    assert rc == OK
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _inputs(dn, n, op, factored):
    comp, vec, _, cells = C.batch(dn, n)
    Gc, gc = G.cotangents(dn, n)
    mat = G.factor_input(dn, n) if factored else comp
    return mat, (None if op == 'factor' else vec), (Gc if op == 'factor' else gc), cells


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_plain_numpy_meets_the_bounds(dn, n):
    """substitutions and products from the definition in the working precision stay under 1 on every judged record
    (or the derivation of a bound is wrong)"""
    assert R.high_ok() and C.judged(dn, n, C.batch(dn, n)[0]).all()
    for factored in (False, True):
        m = G.truth(dn, n, factored)
        for op in G.OPS:
            mat, vec, cot, cells = _inputs(dn, n, op, factored)
            r = G.ratio(dn, m, op, G.plain(dn, n, op, mat, vec, cot, factored), vec, cot)
            print(f'plain {dn} n={n} {op} factored={factored}: {C.worst(r, cells)}')
            assert r.max() <= 1.0, (op, factored, C.worst(r, cells))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_gradients_meet_the_bounds(L, dn, n):
    for factored in (False, True):
        m = G.truth(dn, n, factored)
        for op in G.OPS:
            mat, vec, cot, cells = _inputs(dn, n, op, factored)
            got = host(L, dn, n, op, mat, vec, cot, factored)
            assert np.isfinite(got).all(), (op, factored)
            r = G.ratio(dn, m, op, got, vec, cot)
            print(f'host {dn} n={n} {op} factored={factored}: {C.worst(r, cells)}')
            assert r.max() <= 1.0, (op, factored, C.worst(r, cells))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_factored_route_agrees_with_the_direct_one(L, dn, n):
    """the factor's gradient from the factor the forward routine returns has the bits of the one from the matrix"""
    comp, vec, _, _ = C.batch(dn, n)
    Gc, _ = G.cotangents(dn, n)
    T = R.NP[dn]
    fac = np.full_like(comp, 7.0)
    assert L.nfm_sym_chol_host(DT[dn], n, 0, len(comp), comp.ctypes.data, None, None, fac.ctypes.data) == OK
    assert _same_bits(host(L, dn, n, 'factor', fac, None, Gc, factored=True), host(L, dn, n, 'factor', comp, None, Gc))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_bad_records(L, dn, n):
    """NaN in every value of a bad record's gradient (the four of tests/_symchol_ref.py and a NaN cotangent); the
    neighbours keep their bits"""
    comp, vec, _, _ = C.batch(dn, n)
    Gc, gc = G.cotangents(dn, n)
    at = [0, 63, 64, 199]
    mixed = np.array(comp[:200])
    mixed[at] = C.bad_records(dn, n)
    good = np.setdiff1d(np.arange(200), at + [100])
    for op in G.OPS:
        cot = np.array((Gc if op == 'factor' else gc)[:200])
        clean = host(L, dn, n, op, comp[:200], vec[:200], cot)
        cot[100, -1] = np.nan
        got = host(L, dn, n, op, mixed, vec[:200], cot)
        assert np.isnan(got[at + [100]]).all(), op
        assert _same_bits(got[good], clean[good]) and np.isfinite(got[good]).all(), op
    # a vector that is not finite, an infinite cotangent, and a bad factor handed in as `factored`
    v = np.array(vec[:4])
    v[1, 0], v[2, n - 1] = np.nan, np.inf
    fac = np.array(G.factor_input(dn, n)[:4])
    bad_fac = np.array(fac)
    bad_fac[1, 0], bad_fac[2, 0] = 0.0, -bad_fac[2, 0]
    cot = np.array(gc[:4])
    cot[1, 0] = np.inf
    for op in C.APPLY:
        for got in (host(L, dn, n, op, comp[:4], v, gc[:4]), host(L, dn, n, op, fac, v, gc[:4], factored=True),
                    host(L, dn, n, op, bad_fac, vec[:4], gc[:4], factored=True)):
            assert np.isnan(got[[1, 2]]).all() and np.isfinite(got[[0, 3]]).all(), op
        got = host(L, dn, n, op, comp[:4], vec[:4], cot)
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2, 3]]).all(), op
    got = host(L, dn, n, 'factor', bad_fac, None, Gc[:4], factored=True)
    assert np.isnan(got[[1, 2]]).all() and np.isfinite(got[[0, 3]]).all()


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_factor_gradient_is_scale_equivariant(L, dn, n):
    """for a power of two s the gradient at s^2 A with the same cotangent is the gradient at A divided by s, bit for
    bit, while nothing reaches the subnormals (the 'scaled' cell, already at the edge of the range, is excluded)"""
    comp, _, _, cells = C.batch(dn, n)
    Gc, _ = G.cotangents(dn, n)
    keep = np.ones(len(comp), bool)
    keep[cells['scaled']] = False
    base = host(L, dn, n, 'factor', comp, None, Gc)
    assert np.isfinite(base).all()
    T = R.NP[dn]
    for e in ((-20, 3, 20) if dn == 'f32' else (-200, 7, 200)):
        s = T(2.0) ** T(e)
        got = host(L, dn, n, 'factor', comp[keep] * (s * s), None, Gc[keep])
        assert _same_bits(got, base[keep] / s), e


# ------------------------------------------------------------------------------------------------ CPU tensors
def test_cpu_tensors_facade_and_composition():
    """CPU tensors never reach a kernel: the facade refuses them as before, with and without requires_grad, and the
    torch composition the backward pass differentiates for a second derivative still supports create_graph=True"""
    from nitorch_fastmath_amd import sym as S, _symchol as Y
    comp, vec, _, _ = C.batch('f64', 3)
    a = torch.from_numpy(np.array(comp[:8])).requires_grad_(True)
    v = torch.from_numpy(np.array(vec[:8])).requires_grad_(True)
    for f in (lambda: S.sym_chol(a), lambda: S.sym_chol_apply(a, v, 'L'), lambda: S.sym_chol(a.detach()),
              lambda: S.sym_chol_apply(a.detach(), v, 'Linv', factored=True)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            f()
    with pytest.raises(RuntimeError, match='out='):
        S.sym_chol(a, out=torch.empty(8, 6, dtype=torch.float64))
    for f in (lambda: Y.chol(a), lambda: Y.chol_apply(a, v, 'Linv'), lambda: Y.chol_apply(a, v, 'LTinv', factored=True)):
        res = f()
        (ga,) = torch.autograd.grad(res, a, torch.ones_like(res), create_graph=True)
        assert ga.requires_grad
        (gaa,) = torch.autograd.grad(ga.square().sum(), a)
        assert torch.isfinite(gaa).all() and gaa.abs().max() > 0
