"""CPU-side checks of the Cholesky functions of `sym` (sym_chol, sym_chol_apply, sym_logdet, sym_mahalanobis,
sym_gauss_logpdf): the C ABI's answers without a GPU, the compiled caps and the code-object census, the record routines
the kernels run (`nfm_sym_chol_host`: the same source) against every bound of tests/_symchol_ref.py, forward and
backward, the bad-record rule, the scale equivariance of the factor, the torch composition `_symchol` on CPU tensors
against the model (orders 9 and 12 included), and the facade's argument errors."""
import ctypes
import glob
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _symchol_ref as C
import _symfun_ref as R

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
FACTOR, APPLY, SCALAR, BACKWARD = range(4)              # NFM_CHOL_CLASS_*
FLOOR = {('f32', FACTOR): 8, ('f64', FACTOR): 8, ('f32', APPLY): 8, ('f64', APPLY): 8,
         ('f32', SCALAR): 8, ('f64', SCALAR): 8, ('f32', BACKWARD): 8, ('f64', BACKWARD): 6}
DT = {'f32': 0, 'f64': 1}
NAMES = ('nfm_sym_chol', 'nfm_sym_chol_backward', 'nfm_sym_chol_max_order', 'nfm_sym_chol_host')
FORWARD_OPS = ('factor',) + C.APPLY + C.SCALARS


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
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name]
    assert (_lib.CHOL_FACTOR, _lib.CHOL_LOGDET, _lib.CHOL_MAHA, _lib.CHOL_MAHA_SQRT, _lib.CHOL_LOGPDF) == (0, 5, 6, 7, 8)
    assert _lib.CHOL_APPLY == {'L': 1, 'LT': 2, 'Linv': 3, 'LTinv': 4} and _lib.CHOL_FACTORED == C.FACTORED == 16
    assert (_lib.CHOL_CLASS_FACTOR, _lib.CHOL_CLASS_APPLY, _lib.CHOL_CLASS_SCALAR, _lib.CHOL_CLASS_BACKWARD) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for k, v in (('FACTOR', 0), ('APPLY_L', 1), ('APPLY_LT', 2), ('APPLY_LINV', 3), ('APPLY_LTINV', 4), ('LOGDET', 5),
                 ('MAHA', 6), ('MAHA_SQRT', 7), ('LOGPDF', 8), ('FACTORED', 16), ('CLASS_FACTOR', 0),
                 ('CLASS_APPLY', 1), ('CLASS_SCALAR', 2), ('CLASS_BACKWARD', 3)):
        assert f'#define NFM_CHOL_{k} {v}\n' in hdr
    assert L.nfm_version() == 5


def test_caps_meet_the_floor(L):
    for (dn, cls), floor in FLOOR.items():
        cap = L.nfm_sym_chol_max_order(DT[dn], cls)
        assert floor <= cap <= 8, (dn, cls, cap)
    assert L.nfm_sym_chol_max_order(7, 0) == 0 and L.nfm_sym_chol_max_order(-1, 1) == 0
    assert L.nfm_sym_chol_max_order(0, 4) == 0 and L.nfm_sym_chol_max_order(1, -1) == 0


# (name, C op code, backward, number of operand arguments, index of the operand that may be NULL or None)
ENTRIES = [('factor', 0, False, 3, 1), ('apply', 3, False, 3, None), ('apply_factored', 1 | 16, False, 3, None),
           ('logdet', 5, False, 3, 1), ('maha', 6, False, 3, None), ('logpdf', 8, False, 3, None),
           ('logdet_backward', 5, True, 4, 1), ('maha_backward', 7, True, 4, None), ('logpdf_backward', 8, True, 4, None)]


def _call(L, entry, dtype=0, M=3, op=None, no=1, ni=1, ops=None, ptr=4096):
    from nitorch_fastmath_amd import _lib
    _, code, backward, n_op, _ = entry
    ops = [_lib.Operand(ptr, 0, 1, 0, 1) for _ in range(n_op)] if ops is None else ops
    refs = [None if o is None else ctypes.byref(o) for o in ops]
    fn = L.nfm_sym_chol_backward if backward else L.nfm_sym_chol
    return fn(dtype, M, code if op is None else op, no, ni, *refs, None)


@pytest.mark.parametrize('entry', ENTRIES, ids=[e[0] for e in ENTRIES])
def test_argument_errors_without_a_gpu(L, entry):
    """the canonical bad calls of tests/test_abi_sweep_host.py, the codes and the precedence of nfm_sym_funm, then the
    entry's own checks; every call is refused (or is an empty batch) before any launch"""
    from nitorch_fastmath_amd import _lib
    _, code, backward, n_op, unread = entry
    good = lambda: _lib.Operand(4096, 0, 1, 0, 1)                      # noqa: E731
    assert _call(L, entry, dtype=7) == EDTYPE
    assert _call(L, entry, ni=-1) == EINVAL
    assert _call(L, entry, no=65536) == ESIZE
    assert _call(L, entry, M=0) == ESIZE and _call(L, entry, M=17) == ESIZE
    for k in range(n_op):
        with_k = lambda o: [o if i == k else good() for i in range(n_op)]          # noqa: E731
        if k == unread:            # the op has no vector: the argument is not looked at
            assert _call(L, entry, ni=0, ops=with_k(None)) == OK
            assert _call(L, entry, ni=0, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == OK
            continue
        assert _call(L, entry, ops=with_k(None)) == EINVAL
        assert _call(L, entry, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
        assert _call(L, entry, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    assert _call(L, entry, dtype=7, M=17) == EDTYPE
    assert _call(L, entry, M=17, ops=[None] + [good() for _ in range(n_op - 1)]) == ESIZE
    assert _call(L, entry, dtype=7, ops=[None] + [good() for _ in range(n_op - 1)]) == EDTYPE
    assert _call(L, entry, ni=0, ptr=None) == OK
    # own checks: the op code, then the cap
    bad_ops = [9, 15, 32, -1, 0 | 16, 5 | 16, 8 | 16, 9 | 16] + ([0, 1, 4, 3 | 16] if backward else [])
    for op in bad_ops:
        assert _call(L, entry, op=op) == EINVAL, op
    cls = BACKWARD if backward else (FACTOR if code == 0 else (APPLY if (code & 15) <= 4 else SCALAR))
    for dn in ('f32', 'f64'):
        cap = L.nfm_sym_chol_max_order(DT[dn], cls)
        assert _call(L, entry, dtype=DT[dn], M=cap, ni=0) == OK
        assert _call(L, entry, dtype=DT[dn], M=cap + 1, ni=0) == ESIZE
    assert _call(L, entry, op=9, M=9) == EINVAL          # the op code before the cap
    assert _call(L, entry, op=9, M=17) == ESIZE          # the range of M before the op code


def test_host_entry_argument_errors(L):
    x = np.ones(8)
    p = x.ctypes.data
    H = L.nfm_sym_chol_host
    assert H(7, 2, 0, 1, p, p, None, p) == EDTYPE
    assert H(1, 2, 0, -1, p, p, None, p) == EINVAL
    for op in (9, -1, 32, 0 | 16, 6 | 16):
        assert H(1, 2, op, 1, p, p, None, p) == EINVAL, op
    for op in (0, 1, 4, 3 | 16):                          # no gradient for these
        assert H(1, 2, op, 1, p, p, p, p) == EINVAL, op
    assert H(1, 0, 0, 1, p, p, None, p) == ESIZE and H(1, 9, 0, 1, p, p, None, p) == ESIZE
    assert H(1, 2, 0, 1, None, p, None, p) == EINVAL and H(1, 2, 0, 1, p, p, None, None) == EINVAL
    assert H(1, 2, 6, 1, p, None, None, p) == EINVAL
    assert H(1, 2, 0, 0, None, None, None, None) == OK
    assert H(1, 2, 0, 1, p, None, None, p) == OK and H(1, 2, 5, 1, p, None, None, p) == OK


# ------------------------------------------------------------------------------------------------ the census
def _census():
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_symchol_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_symchol_kernels_in_the_census(L):
    """every (dtype, class, N <= cap) is compiled, none beyond the cap, none with a private segment"""
    rows = _census()
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    names = [k['kernel'] for k in rows]
    for dn, t in (('f32', 'float'), ('f64', 'double')):
        for cls, pats in ((FACTOR, ['CholFactorOp<{t}, {N}>']), (APPLY, ['CholApplyOp<{t}, {N}>']),
                          (SCALAR, ['CholLogdetOp<{t}, {N}>', 'CholQuadOp<{t}, {N}>']),
                          (BACKWARD, ['CholLogdetBwdOp<{t}, {N}>', 'CholQuadBwdOp<{t}, {N}, true>',
                                      'CholQuadBwdOp<{t}, {N}, false>'])):
            cap = L.nfm_sym_chol_max_order(DT[dn], cls)
            for N in range(1, 10):
                for pat in pats:
                    have = any(pat.format(t=t, N=N) in n for n in names)
                    assert have == (N <= cap), (dn, cls, N, cap, pat)


# ------------------------------------------------------------------------------------------------ the record routines
def host(L, dn, n, op, comp, vec=None, g=None, factored=False):
    """`nfm_sym_chol_host` on contiguous numpy records; the result as (nb, size) or (nb,)"""
    T = R.NP[dn]
    comp = np.ascontiguousarray(comp, T)
    nb, K = comp.shape
    vec = None if vec is None else np.ascontiguousarray(vec, T)
    g = None if g is None else np.ascontiguousarray(g, T)
    if g is not None:
        size = K + (0 if op == 'logdet' else n)
    else:
        size = K if op == 'factor' else (n if op in C.APPLY else 1)
    out = np.full((nb, size), 7.0, T)
    rc = L.nfm_sym_chol_host(DT[dn], n, C.CODE[op] | (C.FACTORED if factored else 0), nb, comp.ctypes.data,
                             None if vec is None else vec.ctypes.data, None if g is None else g.ctypes.data,
                             out.ctypes.data)
    assert rc == OK
    return out[:, 0] if size == 1 and g is None and op not in C.APPLY and op != 'factor' else out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_every_record_is_judged(dn, n):
    assert R.high_ok()
    comp = C.batch(dn, n)[0]
    assert len(comp) == C.NB == 1200 and C.judged(dn, n, comp).all(), 'no record of these cells may be excluded'


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_plain_cholesky_meets_the_bounds(dn, n):
    """a plain numpy Cholesky in the working precision stays under 1 on every record (or an input cell is wrong)"""
    comp, vec, g, cells = C.batch(dn, n)
    m, got = C.truth(dn, n), C.plain(dn, comp, vec)
    for op in FORWARD_OPS:
        r = C.forward_ratio(dn, m, op, got[op])
        print(f'plain {dn} n={n} {op}: {C.worst(r, cells)}')
        assert r.max() <= 1.0, (op, C.worst(r, cells))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_forward_meets_the_bounds(L, dn, n):
    comp, vec, g, cells = C.batch(dn, n)
    m = C.truth(dn, n)
    for op in FORWARD_OPS:
        got = host(L, dn, n, op, comp, None if op in ('factor', 'logdet') else vec)
        assert np.isfinite(got).all(), op
        r = C.forward_ratio(dn, m, op, got)
        print(f'host {dn} n={n} {op}: {C.worst(r, cells)}')
        assert r.max() <= 1.0, (op, C.worst(r, cells))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_backward_meets_the_bounds(L, dn, n):
    comp, vec, g, cells = C.batch(dn, n)
    m = C.truth(dn, n)
    for op in C.SCALARS:
        got = host(L, dn, n, op, comp, None if op == 'logdet' else vec, g)
        assert np.isfinite(got).all(), op
        r = C.backward_ratio(dn, m, op, got)
        print(f'host backward {dn} n={n} {op}: {C.worst(r, cells)}')
        assert r.max() <= 1.0, (op, C.worst(r, cells))


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_factored_and_consistency(L, dn, n):
    comp, vec, g, cells = C.batch(dn, n)
    m = C.truth(dn, n)
    fac = host(L, dn, n, 'factor', comp)
    for op in C.APPLY:
        assert _same_bits(host(L, dn, n, op, fac, vec, factored=True), host(L, dn, n, op, comp, vec))
    # Mahalanobis = |L^-1 v|^2 and logpdf = the combination of the other two, within their bounds
    y = host(L, dn, n, 'Linv', comp, vec).astype(R.HP[dn])
    b = C._bounds(dn, m)
    maha = host(L, dn, n, 'maha', comp, vec).astype(R.HP[dn])
    assert (np.abs(maha - (y * y).sum(-1)) <= b['maha']).all()
    logdet = host(L, dn, n, 'logdet', comp).astype(R.HP[dn])
    logpdf = host(L, dn, n, 'logpdf', comp, vec).astype(R.HP[dn])
    assert (np.abs(logpdf + (n * R.HP[dn](C.LOG_2PI) + logdet + maha) / 2) <= b['logpdf']).all()


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_bad_records(L, dn, n):
    """NaN in every value of a bad record, forward and backward; the neighbours keep their bits"""
    comp, vec, g, _ = C.batch(dn, n)
    bad = C.bad_records(dn, n)
    at = [0, 63, 64, 199]
    mixed = np.array(comp[:200])
    mixed[at] = bad
    good = np.setdiff1d(np.arange(200), at)
    for op in FORWARD_OPS:
        v = None if op in ('factor', 'logdet') else vec[:200]
        got, clean = host(L, dn, n, op, mixed, v), host(L, dn, n, op, comp[:200], v)
        assert np.isnan(got[at]).all(), op
        assert _same_bits(got[good], clean[good]), op
    for op in C.SCALARS:
        v = None if op == 'logdet' else vec[:200]
        got, clean = host(L, dn, n, op, mixed, v, g[:200]), host(L, dn, n, op, comp[:200], v, g[:200])
        assert np.isnan(got[at]).all(), op
        assert _same_bits(got[good], clean[good]), op
    # a vector that is not finite makes its record bad; a bad factor handed in as `factored` too
    v = np.array(vec[:4])
    v[1, 0], v[2, n - 1] = np.nan, np.inf
    for op in C.APPLY + ('maha', 'maha_sqrt', 'logpdf'):
        got = host(L, dn, n, op, comp[:4], v)
        assert np.isnan(got[[1, 2]]).all() and np.isfinite(got[[0, 3]]).all(), op
    fac = host(L, dn, n, 'factor', comp[:4])
    fac[1, 0], fac[2, 0] = 0.0, -fac[2, 0]
    for op in C.APPLY:
        got = host(L, dn, n, op, fac, vec[:4], factored=True)
        assert np.isnan(got[[1, 2]]).all() and np.isfinite(got[[0, 3]]).all(), op
    # a singular record: NaN, not -inf
    sing = bad[1:2]
    assert np.isnan(host(L, dn, n, 'logdet', sing)).all()


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_root_gradient_at_zero(L, dn, n):
    comp, vec, g, _ = C.batch(dn, n)
    got = host(L, dn, n, 'maha_sqrt', comp[:64], np.zeros_like(vec[:64]), g[:64])
    assert (got == 0).all()


@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_factor_is_scale_equivariant(L, dn, n):
    """chol(s^2 A) == s chol(A) bit for bit for a power of two s while nothing reaches the subnormals"""
    comp, _, _, cells = C.batch(dn, n)
    keep = np.ones(len(comp), bool)
    keep[cells['scaled']] = False                       # already at the edge of the range: scaled on their own below
    base = host(L, dn, n, 'factor', comp)
    assert np.isfinite(base).all()
    T = R.NP[dn]
    for e in ((-20, 3, 20) if dn == 'f32' else (-200, 7, 200)):
        s = T(2.0) ** T(e)
        got = host(L, dn, n, 'factor', comp[keep] * (s * s))
        assert _same_bits(got, base[keep] * s), e
    e = 4 if dn == 'f32' else 40
    s = T(2.0) ** T(e)
    for sign in (1, -1):
        sl = cells['scaled']
        got = host(L, dn, n, 'factor', comp[sl] * (s * s if sign > 0 else 1 / (s * s)))
        assert _same_bits(got, base[sl] * (s if sign > 0 else 1 / s))


# ------------------------------------------------------------------------------------------------ the torch route
def _route_batch(dn, n):
    """128 records of every cell kind at an order the kernels do not serve too (the model works at any order)"""
    rng = np.random.default_rng(900 + n)
    parts = [C.cell(c, dn, rng, 16, n) for c in C.CELLS]
    comp = R.pack(np.concatenate(parts)).astype(R.NP[dn])
    vec = rng.standard_normal((len(comp), n)).astype(R.NP[dn])
    g = rng.standard_normal(len(comp)).astype(R.NP[dn])
    return comp, vec, g


@pytest.mark.parametrize('n', [3, 9, 12])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_route_meets_the_bounds_on_cpu(dn, n):
    from nitorch_fastmath_amd import _symchol as Y
    comp, vec, g = _route_batch(dn, n)
    assert C.judged(dn, n, comp).all()
    m = C.model(dn, comp, vec, g)
    tc, tv, tg = torch.from_numpy(comp), torch.from_numpy(vec), torch.from_numpy(g)
    fwd = {'factor': lambda a, v: Y.chol(a), 'logdet': lambda a, v: Y.logdet(a),
           'maha': lambda a, v: Y.mahalanobis(a, v), 'maha_sqrt': lambda a, v: Y.mahalanobis(a, v, squared=False),
           'logpdf': Y.gauss_logpdf}
    for op in C.APPLY:
        fwd[op] = lambda a, v, op=op: Y.chol_apply(a, v, op)
    for op in FORWARD_OPS:
        r = C.forward_ratio(dn, m, op, fwd[op](tc, tv).numpy())
        assert r.max() <= 1.0, (op, float(r.max()))
    fac = Y.chol(tc)
    for op in C.APPLY:
        r = C.forward_ratio(dn, m, op, Y.chol_apply(fac, tv, op, factored=True).numpy())
        assert r.max() <= 1.0, (op, float(r.max()))
    for op in C.SCALARS:
        a, v = tc.clone().requires_grad_(True), tv.clone().requires_grad_(True)
        fwd[op](a, v).backward(tg)
        packed = a.grad.numpy() if op == 'logdet' else np.concatenate([a.grad.numpy(), v.grad.numpy()], -1)
        r = C.backward_ratio(dn, m, op, packed)
        assert r.max() <= 1.0, (op, float(r.max()))


def test_route_bad_records_and_zero_distance():
    from nitorch_fastmath_amd import _symchol as Y
    n = 9
    comp, vec, g = _route_batch('f64', n)
    comp, vec, g = np.array(comp[:8]), np.array(vec[:8]), g[:8]
    comp[[1, 3, 5, 6]] = C.bad_records('f64', n)
    vec[7] = 0.0
    tg = torch.from_numpy(g)
    good = [0, 2, 4, 7]
    for f, with_vec in ((Y.chol, False), (Y.logdet, False), (Y.mahalanobis, True), (Y.gauss_logpdf, True),
                        (lambda a, v: Y.mahalanobis(a, v, squared=False), True),
                        (lambda a, v: Y.chol_apply(a, v, 'Linv'), True)):
        a = torch.from_numpy(comp).requires_grad_(True)
        v = torch.from_numpy(vec).requires_grad_(True)
        res = f(a, v) if with_vec else f(a)
        res.backward(tg if res.dim() == 1 else tg[:, None].expand_as(res))
        flat = res.detach().reshape(8, -1).numpy()
        assert np.isnan(flat[[1, 3, 5, 6]]).all() and np.isfinite(flat[good]).all()
        grads = [a.grad.numpy()] + ([v.grad.numpy()] if with_vec else [])
        for gr in grads:
            assert np.isnan(gr[[1, 3, 5, 6]]).all() and np.isfinite(gr[good]).all()
    a = torch.from_numpy(comp).requires_grad_(True)
    v = torch.from_numpy(vec).requires_grad_(True)
    Y.mahalanobis(a, v, squared=False).backward(tg)
    assert (a.grad[7] == 0).all() and (v.grad[7] == 0).all()


def test_route_gradcheck():
    from nitorch_fastmath_amd import _symchol as Y
    comp, vec, _ = _route_batch('f64', 3)
    a = torch.from_numpy(np.array(comp[:4])).requires_grad_(True)
    v = torch.from_numpy(np.array(vec[:4])).requires_grad_(True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(Y.chol, (a,), **kw)
    assert torch.autograd.gradcheck(Y.logdet, (a,), **kw)
    assert torch.autograd.gradcheck(Y.gauss_logpdf, (a, v), **kw)
    assert torch.autograd.gradcheck(lambda x, y: Y.mahalanobis(x, y, squared=False), (a, v), **kw)
    assert torch.autograd.gradcheck(lambda x, y: Y.chol_apply(x, y, 'LTinv'), (a, v), **kw)


# ------------------------------------------------------------------------------------------------ the facade
def test_facade_rejects_bad_arguments():
    import nitorch_fastmath_amd as N
    from nitorch_fastmath_amd import sym as S
    names = ('sym_chol', 'sym_chol_apply', 'sym_logdet', 'sym_mahalanobis', 'sym_gauss_logpdf')
    for name in names:
        assert name in S.__all__ and getattr(N, name) is getattr(S, name)
    x, v = torch.ones(4, 6), torch.ones(4, 3)
    calls = {'sym_chol': lambda a, **kw: S.sym_chol(a, **kw), 'sym_logdet': lambda a, **kw: S.sym_logdet(a, **kw),
             'sym_chol_apply': lambda a, b=v, **kw: S.sym_chol_apply(a, b, 'Linv', **kw),
             'sym_mahalanobis': lambda a, b=v, **kw: S.sym_mahalanobis(a, b, **kw),
             'sym_gauss_logpdf': lambda a, b=v, **kw: S.sym_gauss_logpdf(a, b, **kw)}
    for name, f in calls.items():
        with pytest.raises(ValueError, match='not M\\*\\(M\\+1\\)/2'):
            f(torch.ones(4, 5))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            f(x)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            f(x.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match='out='):
            f(x.clone().requires_grad_(True), out=torch.empty(4))
        if name not in ('sym_chol', 'sym_logdet'):
            with pytest.raises(ValueError, match='components'):
                f(x, torch.ones(4, 4))
    for op in ('l', 'Lt', 'inv', None):
        with pytest.raises(ValueError, match='op must be'):
            S.sym_chol_apply(x, v, op)
