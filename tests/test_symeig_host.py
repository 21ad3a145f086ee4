"""CPU-side checks of `sym.sym_eigvals` / `sym.sym_eigh` (sorted eigendecomposition of compact symmetric matrices):
the C ABI's answers without a GPU, the compiled caps and the code-object census, the sort, the sign rule and the gap
weights the kernels apply (`nfm_sym_eigh_host_finish`: the source they run) against numpy, the torch route `_symeig`
on CPU tensors against the model of tests/_symeig_ref.py, and the facade's argument errors."""
import ctypes
import glob
import itertools
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _eig_ref as E
import _symeig_ref as Q
import _symfun_ref as R

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
VALUES, VECTORS, VALUES_BACKWARD, BACKWARD = range(4)
FLOOR = {('f32', VALUES): 8, ('f64', VALUES): 8, ('f32', VECTORS): 8, ('f64', VECTORS): 6,       # the required orders
         ('f32', VALUES_BACKWARD): 8, ('f64', VALUES_BACKWARD): 6, ('f32', BACKWARD): 6, ('f64', BACKWARD): 4}
DT = {'f32': 0, 'f64': 1}
ORDER = {'ascending': 0, 'descending': 1, 'abs': 2}
NAMES = ('nfm_sym_eigh', 'nfm_sym_eigh_backward', 'nfm_sym_eigh_max_order', 'nfm_sym_eigh_host_finish')


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
    assert _lib.EIGH_ORDER == ORDER and _lib.EIGH_VECTORS == 4
    assert (_lib.EIGH_OP_VALUES, _lib.EIGH_OP_VECTORS, _lib.EIGH_OP_VALUES_BACKWARD, _lib.EIGH_OP_BACKWARD) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for k, v in ORDER.items():
        assert f'#define NFM_EIGH_{k.upper()} {v}\n' in hdr
    for k, v in (('VECTORS', 4), ('OP_VALUES', 0), ('OP_VECTORS', 1), ('OP_VALUES_BACKWARD', 2), ('OP_BACKWARD', 3)):
        assert f'#define NFM_EIGH_{k} {v}\n' in hdr


def test_caps_meet_the_floor(L):
    for (dn, op), floor in FLOOR.items():
        cap = L.nfm_sym_eigh_max_order(DT[dn], op)
        assert floor <= cap <= 8, (dn, op, cap)
    assert L.nfm_sym_eigh_max_order(7, 0) == 0 and L.nfm_sym_eigh_max_order(-1, 1) == 0
    assert L.nfm_sym_eigh_max_order(0, 4) == 0 and L.nfm_sym_eigh_max_order(1, -1) == 0


def _n_op(op):
    return {VALUES: 2, VECTORS: 2, VALUES_BACKWARD: 3, BACKWARD: 4}[op]


def _call(L, op, dtype=0, M=3, flags=0, no=1, ni=1, ops=None, ptr=4096):
    """the entry of `op` with its operands in argument order (values backward: mat, gval, gmat; gvec = NULL)"""
    from nitorch_fastmath_amd import _lib
    ops = [_lib.Operand(ptr, 0, 1, 0, 1) for _ in range(_n_op(op))] if ops is None else ops
    refs = [None if o is None else ctypes.byref(o) for o in ops]
    if op == VALUES:
        return L.nfm_sym_eigh(dtype, M, flags, no, ni, *refs, None)
    if op == VECTORS:
        return L.nfm_sym_eigh(dtype, M, flags | 4, no, ni, *refs, None)
    if op == VALUES_BACKWARD:
        return L.nfm_sym_eigh_backward(dtype, M, flags, no, ni, refs[0], refs[1], None, refs[2], None)
    return L.nfm_sym_eigh_backward(dtype, M, flags | 4, no, ni, *refs, None)


@pytest.mark.parametrize('op', [VALUES, VECTORS, VALUES_BACKWARD, BACKWARD])
def test_argument_errors_without_a_gpu(L, op):
    """the canonical bad calls of tests/test_abi_sweep_host.py, the codes and the precedence of nfm_sym_funm, then the
    entry's own checks; every call is refused (or is an empty batch) before any launch"""
    from nitorch_fastmath_amd import _lib
    n_op = _n_op(op)
    good = lambda: _lib.Operand(4096, 0, 1, 0, 1)                      # noqa: E731
    assert _call(L, op, dtype=7) == EDTYPE
    assert _call(L, op, ni=-1) == EINVAL
    assert _call(L, op, no=65536) == ESIZE
    assert _call(L, op, M=0) == ESIZE and _call(L, op, M=17) == ESIZE
    for k in range(n_op):
        with_k = lambda o: [o if i == k else good() for i in range(n_op)]          # noqa: E731
        if not (op == BACKWARD and k == 2):        # a NULL gvec is the values-only call, not an error
            assert _call(L, op, ops=with_k(None)) == EINVAL
        assert _call(L, op, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
        assert _call(L, op, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    assert _call(L, op, dtype=7, M=17) == EDTYPE
    assert _call(L, op, M=17, ops=[None] + [good() for _ in range(n_op - 1)]) == ESIZE
    assert _call(L, op, dtype=7, ops=[None] + [good() for _ in range(n_op - 1)]) == EDTYPE
    assert _call(L, op, ni=0, ptr=None) == OK
    # own checks: the order code, then the cap
    for flags in (3, 8, 16, -1):
        assert _call(L, op, flags=flags) == EINVAL, flags
    for flags in (0, 1, 2):
        assert _call(L, op, flags=flags, ni=0) == OK
    for dn in ('f32', 'f64'):
        cap = L.nfm_sym_eigh_max_order(DT[dn], op)
        assert _call(L, op, dtype=DT[dn], M=cap, ni=0) == OK
        assert _call(L, op, dtype=DT[dn], M=cap + 1, ni=0) == ESIZE
    assert _call(L, op, flags=3, M=9) == EINVAL          # the order code before the cap
    assert _call(L, op, flags=3, M=17) == ESIZE          # the range of M before the order code


def test_host_finish_argument_errors(L):
    x = np.ones(4)
    p = x.ctypes.data
    assert L.nfm_sym_eigh_host_finish(7, 0, 2, 1, p, p, p) == EDTYPE
    assert L.nfm_sym_eigh_host_finish(1, 3, 2, 1, p, p, p) == EINVAL
    assert L.nfm_sym_eigh_host_finish(1, -1, 2, 1, p, p, p) == EINVAL
    assert L.nfm_sym_eigh_host_finish(1, 0, 2, -1, p, p, p) == EINVAL
    assert L.nfm_sym_eigh_host_finish(1, 0, 0, 1, p, p, p) == ESIZE
    assert L.nfm_sym_eigh_host_finish(1, 0, 9, 1, p, p, p) == ESIZE
    assert L.nfm_sym_eigh_host_finish(1, 0, 2, 1, None, p, p) == EINVAL
    assert L.nfm_sym_eigh_host_finish(1, 0, 2, 0, None, None, None) == OK
    assert L.nfm_sym_eigh_host_finish(1, 0, 2, 1, p, None, None) == OK


# ------------------------------------------------------------------------------------------------ the census
def _census():
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_symeig_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_symeig_kernels_in_the_census(L):
    """every (dtype, op, N <= cap) is compiled, none beyond the cap, none with a private segment"""
    rows = _census()
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    names = [k['kernel'] for k in rows]
    for dn, t in (('f32', 'float'), ('f64', 'double')):
        for op, pat in ((VALUES, 'SymEigOp<{t}, {N}, false>'), (VECTORS, 'SymEigOp<{t}, {N}, true>'),
                        (VALUES_BACKWARD, 'SymEigValBwdOp<{t}, {N}>'), (BACKWARD, 'SymEigBwdOp<{t}, {N}>')):
            cap = L.nfm_sym_eigh_max_order(DT[dn], op)
            for N in range(1, 10):
                have = any(pat.format(t=t, N=N) in n for n in names)
                assert have == (N <= cap), (dn, op, N, cap)


# ------------------------------------------------------------------------------------------------ sort, signs, gaps
def _finish(L, dn, order, lam, vec=None, want_w=False):
    lam = np.array(lam, R.NP[dn], order='C')
    nb, n = lam.shape
    vec = None if vec is None else np.array(vec, R.NP[dn], order='C')
    w = np.full((nb, n, n), 7.0, R.NP[dn]) if want_w else None
    rc = L.nfm_sym_eigh_host_finish(DT[dn], ORDER[order], n, nb, lam.ctypes.data,
                                    None if vec is None else vec.ctypes.data, None if w is None else w.ctypes.data)
    assert rc == OK
    return lam, vec, w


def _finish_records(dn, n, rng):
    """64 spectra with ties, +-x pairs, zeros and -0.0, and 64 random vector matrices with magnitude ties"""
    T = R.NP[dn]
    pool = np.array([0.0, -0.0, 1.0, -1.0, 2.5, -2.5, 2.5, 1e-30, -1e-30, 3.0], np.float64)
    lam = rng.standard_normal((64, n))
    lam[:40] = pool[rng.integers(0, len(pool), (40, n))]
    lam[40:48] = np.round(lam[40:48] * 2) / 2                  # many exact ties and +-x pairs
    lam[48] = 0.0
    lam[49] = -0.0
    vec = rng.standard_normal((64, n, n))
    vec[:16] = np.round(vec[:16] * 2) / 2                       # exact ties of the largest magnitude
    vec[16:24] = -np.abs(vec[16:24])
    return lam.astype(T), vec.astype(T)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize('order', Q.ORDERS)
@pytest.mark.parametrize('n', range(1, 9))
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_finish_sorts_and_fixes_signs(L, dn, n, order):
    rng = np.random.default_rng(100 * n + ORDER[order])
    lam, vec = _finish_records(dn, n, rng)
    idx = Q.sort_index(lam, order)
    want_lam = np.take_along_axis(lam, idx, -1)
    got_lam, got_vec, _ = _finish(L, dn, order, lam, vec)
    assert _same_bits(got_lam, want_lam)                       # the exact order, -0.0 and +0.0 told apart
    assert Q.is_sorted(got_lam, order).all()
    only_lam, _, _ = _finish(L, dn, order, lam)
    assert _same_bits(only_lam, want_lam)
    # columns travel with their values: where the values are distinct the permutation is known
    want_vec = Q.fix_signs(np.take_along_axis(vec, idx[:, None, :], -1))
    distinct = np.array([len(set(r.tobytes()[i * r.itemsize:(i + 1) * r.itemsize] for i in range(n))) == n for r in lam])
    assert distinct.sum() >= 14                                # the 14 random records at least
    assert _same_bits(got_vec[distinct], want_vec[distinct])
    # everywhere: the columns are a permutation of the input's, up to sign, and the sign rule holds
    assert Q.signs_ok(got_vec)[(np.abs(got_vec).max(-2) > 0).all(-1)].all()
    for b in range(64):
        a = sorted(np.abs(vec[b]).T.tolist())
        assert a == sorted(np.abs(got_vec[b]).T.tolist())
    top = np.argmax(np.abs(got_vec), -2)
    assert (np.take_along_axis(got_vec, top[:, None, :], -2) >= 0).all()


@pytest.mark.parametrize('n', range(2, 9))
def test_sort_network_by_the_zero_one_principle(L, n):
    """a compare-exchange network that sorts every 0/1 input sorts every input"""
    lam = np.array(list(itertools.product([0.0, 1.0], repeat=n)))
    for order in Q.ORDERS:
        got, _, _ = _finish(L, 'f64', order, lam if order != 'descending' else -lam)
        assert Q.is_sorted(got, order).all()
        assert np.array_equal(np.sort(np.abs(got), -1), np.sort(lam, -1))


@pytest.mark.parametrize('n', range(1, 9))
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_finish_gap_weights(L, dn, n):
    T = R.NP[dn]
    eps = R.eps_of(dn)
    rng = np.random.default_rng(300 + n)
    lam = rng.standard_normal((64, n))
    lam[:8] = 1.0                                               # isotropic
    lam[8:16, : n // 2] = -0.5                                  # repeated
    lam[8:16, n // 2:] = 1.0
    lam[16:24] = 1.0 + 1e-6 * rng.standard_normal((8, n))
    k = np.arange(8.0)[:, None]
    lam[24:32] = 1.0 + (4.0 * n * eps) * k * np.arange(n)      # spacings of 0, 4, 8, ... n eps: both sides of 16 n eps
    lam[32:40] = 0.0
    lam = lam.astype(T)
    got_lam, _, w = _finish(L, dn, 'ascending', lam, want_w=True)
    want, close = Q.gap_weights(got_lam)
    assert _same_bits(w, want)
    assert (w[close] == 0).all() and np.isfinite(w).all()
    assert (w[~close] != 0).all()
    if n > 1:
        off = ~np.eye(n, dtype=bool)
        assert close[:8][:, off].all() and close[32:40][:, off].all()
        assert close[24:32][:, off].any() and not close[24:32][:, off].all()
        assert not close[40:][:, off].any()


# ------------------------------------------------------------------------------------------------ the torch route
def _route(comp, order, gl=None, gv=None, vectors=True):
    from nitorch_fastmath_amd import _symeig
    x = torch.from_numpy(np.array(comp)).requires_grad_(gl is not None or gv is not None)
    res = _symeig.sym_eigh(x, ORDER[order], vectors)
    lam, V = res if vectors else (res, None)
    if x.requires_grad:
        outs, grads = [], []
        if gl is not None:
            outs.append(lam)
            grads.append(torch.from_numpy(np.array(gl)))
        if gv is not None:
            outs.append(V)
            grads.append(torch.from_numpy(np.array(gv)))
        torch.autograd.backward(outs, grads)
    return (lam.detach().numpy(), None if V is None else V.detach().numpy(),
            None if x.grad is None else x.grad.numpy())


@pytest.mark.parametrize('order', Q.ORDERS)
@pytest.mark.parametrize('n', [3, 9])
def test_route_forward_meets_the_bars_on_cpu(n, order):
    a = E.batch('f64', n)[0]
    comp = R.pack(a)
    vals, _, _ = _route(comp, order, vectors=False)
    vals_u, vecs, _ = _route(comp, order)
    E.assert_records_within('f64', n, a, vals, vals_u, vecs)
    assert Q.is_sorted(vals, order).all() and Q.is_sorted(vals_u, order).all()
    nz = (np.abs(vecs).max(-2) > 0).all(-1)
    assert nz.all() and Q.signs_ok(vecs).all()


@pytest.mark.parametrize('n', [2, 3, 5, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_route_gradients_within_the_bounds_on_cpu(dn, n):
    """the torch route on CPU tensors: LAPACK in the working dtype.  It must stay below C / 4 (or the conditioning
    expression of tests/_symeig_ref.py is wrong)"""
    assert R.high_ok()
    full, comp, cells = Q.grad_batch(dn, n)
    gl, gv = Q.cotangents(dn, n, len(full))
    _, vecs, _ = _route(comp, 'ascending')
    mod = Q.model(dn, full, 'ascending', vecs, gl, gv, hp=Q._eigh_hp(dn, n))
    assert Q.judged(dn, n, mod).all(), 'no record of these cells may be excluded'
    worst = {}
    for name, a, b in (('values', gl, None), ('vectors', None, gv), ('both', gl, gv)):
        _, _, gx = _route(comp, 'ascending', a, b)
        assert np.isfinite(gx).all()
        r = Q.grad_ratio(dn, n, mod, gx, a, b)
        worst[name] = {c: float(r[sl].max()) for c, sl in cells.items()}
    print(f'{dn} n={n}: {worst} (of {Q.C}); smallest gap/|A| {float((mod["gap"] / mod["norm"]).min()):.2e}')
    assert max(max(v.values()) for v in worst.values()) <= Q.C / 4, worst


def test_route_gradients_follow_the_order():
    """'descending' and 'abs' permute the cotangents with the eigenpairs"""
    full, comp, _ = Q.grad_batch('f64', 5)
    gl, gv = Q.cotangents('f64', 5, len(full))
    for order in ('descending', 'abs'):
        _, vecs, gx = _route(comp, order, gl, gv)
        mod = Q.model('f64', full, order, vecs, gl, gv, hp=Q._eigh_hp('f64', 5))
        assert Q.grad_ratio('f64', 5, mod, gx, gl, gv).max() <= Q.C / 4


def test_route_gradcheck():
    from nitorch_fastmath_amd import _symeig
    comp = Q.grad_batch('f64', 3)[1]
    x = torch.from_numpy(np.array(comp[:4])).requires_grad_(True)              # 4 `normal` records

    def loss(t):                                                                # invariant to the vectors' signs
        lam, V = _symeig.sym_eigh(t, 0, True)
        return lam, V[..., :, None, :] * V[..., None, :, :]

    assert torch.autograd.gradcheck(loss, (x,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda t: _symeig.sym_eigh(t, 2, False), (x,), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize('n', [3, 6])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_route_gradients_are_finite_on_degenerate_spectra(dn, n):
    comp, cells = R.batch(dn, n, 'log', nb=7 * 16)
    gl, gv = Q.cotangents(dn, n, len(comp))
    for fam in ('isotropic', 'repeated', 'cluster'):
        sl = cells[fam]
        for a, b in ((gl[sl], None), (None, gv[sl]), (gl[sl], gv[sl])):
            _, _, gx = _route(comp[sl], 'ascending', a, b)
            assert np.isfinite(gx).all(), (fam, a is None, b is None)
        # gl = 1: S = V V^T = I
        _, _, gx = _route(comp[sl], 'ascending', np.ones_like(gl[sl]), None)
        s = R.unpack(gx, n, off=0.5)
        assert np.abs(s - np.eye(n)).max() <= Q.C * n * n * R.eps_of(dn), fam


def test_route_nan_records():
    comp = np.array(Q.grad_batch('f64', 3)[1][:5])
    comp[1, 4] = np.nan
    comp[3, 0] = np.inf
    gl, gv = Q.cotangents('f64', 3, 5)
    lam, V, gx = _route(comp, 'abs', gl, gv)
    for r in (lam, V.reshape(5, -1), gx):
        assert np.isnan(r[[1, 3]]).all() and np.isfinite(r[[0, 2, 4]]).all()
    lam2, V2, gx2 = _route(comp[[0, 2, 4]], 'abs', gl[[0, 2, 4]], gv[[0, 2, 4]])
    assert np.array_equal(lam[[0, 2, 4]], lam2) and np.array_equal(V[[0, 2, 4]], V2)
    assert np.array_equal(gx[[0, 2, 4]], gx2)


# ------------------------------------------------------------------------------------------------ the facade
def test_facade_rejects_bad_arguments():
    import nitorch_fastmath_amd as N
    from nitorch_fastmath_amd import sym as S
    for name in ('sym_eigvals', 'sym_eigh'):
        assert name in S.__all__ and getattr(N, name) is getattr(S, name)
    x = torch.ones(4, 6)
    for f in (S.sym_eigvals, S.sym_eigh):
        with pytest.raises(ValueError, match='order must be'):
            f(x, order='largest')
        with pytest.raises(ValueError, match='not M\\*\\(M\\+1\\)/2'):
            f(torch.ones(4, 5))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            f(x)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            f(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='out='):
        S.sym_eigvals(x.clone().requires_grad_(True), out=torch.empty(4, 3))
    with pytest.raises(TypeError):
        S.sym_eigh(x, out=torch.empty(4, 3))
