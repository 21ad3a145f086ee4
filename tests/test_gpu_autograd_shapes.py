"""Backward passes at sizes where a wave tail and a tile exist, in both dtypes, at every order, and on the
operand combinations that only a backward produces (a transposed full matrix, an expanded stride-0 cotangent,
a broadcast matrix at orders 9..16, eps, dtype=, pivoting=).

Truth: torch's autograd of the dense equivalent on the CPU, in float64 on the upcast inputs.  float64 results
are held to rtol 1e-9 / atol 1e-11 against it.  float32 results are held to the error model of conftest.py
against the same dense computation in CPU float32 (the reference): err(got) <= 2 err(ref) + 4 M eps."""
import numpy as np
import pytest
import torch
from conftest import TOL, relerr, model_bound
import _dense_ref as R

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}
N197 = 197                                   # 3 wavefronts + 5


def N():
    import nitorch_fastmath_amd as N_
    return N_


def sizes(M):
    return (N197, 1000 + M) if M >= 9 else (N197,)


# ---- differentiable dense equivalents (plain torch, CPU) ---------------------------------------------------
def to_full(c, M):
    rows = [[None] * M for _ in range(M)]
    for k, (i, j) in enumerate(R.pairs(M)):
        rows[i][j] = rows[j][i] = c[..., k]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def compact(full):
    return torch.stack([full[..., i, j] for i, j in R.pairs(full.shape[-1])], -1)


def eps_vector(eps, M, like):
    e = list(eps) if isinstance(eps, (list, tuple)) else [eps]
    return torch.tensor((e + [e[-1]] * M)[:M], dtype=like.dtype)


def dense_solve(M, storage='sym', eps=None):
    def fn(mat, vec):
        if storage == 'diag':
            return vec / (mat if eps is None else mat + eps_vector(eps, M, mat))
        A = mat.unflatten(-1, (M, M)) if storage == 'full' else to_full(mat, M)
        if eps is not None:
            A = A + torch.diag_embed(eps_vector(eps, M, mat))
        batch = torch.broadcast_shapes(A.shape[:-2], vec.shape[:-1])
        return torch.linalg.solve(A.expand(batch + (M, M)), vec.expand(batch + (M,)).unsqueeze(-1)).squeeze(-1)
    return fn


def dense_matvec(M, mode):
    def fn(mat, vec, inp=None):
        y = (to_full(mat, M) @ vec.unsqueeze(-1)).squeeze(-1)
        return y if mode == 0 else inp + mode * y
    return fn


# ---- the harness -------------------------------------------------------------------------------------------
def as_is(x):
    return x


def channel_first(x):
    """(n, C) stored (C, n): a non-contiguous leaf"""
    return x.t().contiguous().t()


def gradients(fn, leaves, weight):
    out = fn(*leaves)
    ((out * weight).sum() if weight is not None else out.sum()).backward()
    return out.detach(), [x.grad for x in leaves]


def check_backward(dev, dn, M, gpu_fn, dense_fn, arrays, weighted=True, place=None, seed=0, what=''):
    """gradients of every array of `arrays` (numpy, already of the dtype under test) through `gpu_fn` on the
    device against `dense_fn` on the CPU; `weighted=False` is `.sum().backward()`, whose cotangent reaches the
    backward as an expanded stride-0 tensor"""
    place = place or [as_is] * len(arrays)
    leaves64 = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in arrays]
    with torch.no_grad():
        shape = dense_fn(*leaves64).shape
    w = np.random.default_rng(seed + 12345).standard_normal(tuple(shape)).astype(R.NP[dn]) if weighted else None
    _, truth = gradients(dense_fn, leaves64, None if w is None else torch.from_numpy(w.astype(np.float64)))
    if dn == 'f32':
        leaves32 = [torch.from_numpy(a.copy()).requires_grad_() for a in arrays]
        _, ref = gradients(dense_fn, leaves32, None if w is None else torch.from_numpy(w))
    leaves = [p(torch.from_numpy(a.copy()).to(dev)).detach().requires_grad_() for p, a in zip(place, arrays)]
    out, got = gradients(gpu_fn, leaves, None if w is None else torch.from_numpy(w).to(dev))
    assert tuple(out.shape) == tuple(shape)
    for k, (g, tr) in enumerate(zip(got, truth)):
        assert g is not None and g.dtype == DT[dn] and g.shape == tr.shape, (what, k)
        g = g.cpu()
        assert bool(torch.isfinite(g).all()), (what, k)
        if dn == 'f64':
            assert torch.allclose(g, tr, rtol=1e-9, atol=1e-11), (what, k, relerr(g, tr))
        else:
            e_got, e_ref, bound = relerr(g, tr), relerr(ref[k], tr), model_bound(ref[k], tr, M, 'f32')
            print(f'{what} M={M} leaf {k}: err(got) {e_got:.3g} err(ref) {e_ref:.3g} bound {bound:.3g}')
            assert e_got <= bound, (what, k, e_got, e_ref, bound)


def inputs(n, M, dn, seed):
    mat, vec = R.spd_np(n, M, R.NP[dn], seed)
    inp = np.random.default_rng(seed + 1).standard_normal((n, M)).astype(R.NP[dn])
    return mat, vec, inp


# =========================================================================== sym_solve / matvec family
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', R.ORDERS)
def test_solve_and_matvec_backward_every_order(dev, dn, M):
    S = N().sym
    for n in sizes(M):
        mat, vec, inp = inputs(n, M, dn, 100 * M + n)
        for weighted in (True, False):
            check_backward(dev, dn, M, S.sym_solve, dense_solve(M), [mat, vec], weighted, what='sym_solve')
            check_backward(dev, dn, M, S.sym_matvec, dense_matvec(M, 0), [mat, vec], weighted, what='sym_matvec')
            check_backward(dev, dn, M, lambda m, v, i: S.sym_addmatvec(i, m, v), dense_matvec(M, +1),
                           [mat, vec, inp], weighted, what='sym_addmatvec')
            check_backward(dev, dn, M, lambda m, v, i: S.sym_submatvec(i, m, v), dense_matvec(M, -1),
                           [mat, vec, inp], weighted, what='sym_submatvec')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', [3, 6, 9, 16])
def test_solve_backward_variants(dev, dn, M):
    S = N().sym
    K = M * (M + 1) // 2
    for n in sizes(M):
        mat, vec, _ = inputs(n, M, dn, 200 * M + n)
        rng = np.random.default_rng(M + n)
        for weighted in (True, False):
            eps = [0.5, 0.25]
            check_backward(dev, dn, M, lambda m, v: S.sym_solve(m, v, eps=eps), dense_solve(M, eps=eps),
                           [mat, vec], weighted, what='eps')
            # diagonal and full-matrix storage (the backward solves with the TRANSPOSED full matrix: not symmetric)
            check_backward(dev, dn, M, S.sym_solve, dense_solve(M, 'diag'), [np.ascontiguousarray(mat[:, :M]), vec],
                           weighted, what='diag')
            check_backward(dev, dn, M, lambda m, v: S.sym_solve(m, v, eps=eps), dense_solve(M, 'diag', eps),
                           [np.ascontiguousarray(mat[:, :M]), vec], weighted, what='diag eps')
            full = R.to_full(mat) + 0.25 / np.sqrt(M) * rng.standard_normal((n, M, M))
            full = full.reshape(n, M * M).astype(R.NP[dn])
            check_backward(dev, dn, M, S.sym_solve, dense_solve(M, 'full'), [full, vec], weighted, what='full')
            check_backward(dev, dn, M, S.sym_matvec,
                           lambda m, v: (m.unflatten(-1, (M, M)) @ v.unsqueeze(-1)).squeeze(-1),
                           [full, vec], weighted, what='full matvec')
            # channel-first leaves
            check_backward(dev, dn, M, S.sym_solve, dense_solve(M), [mat, vec], weighted,
                           place=[channel_first, channel_first], what='channel-first')
            # one matrix against n vectors (grad summed over the batch; M >= 9: the broadcast kernel in the backward
            # solve), one vector against n matrices
            check_backward(dev, dn, M, S.sym_solve, dense_solve(M), [mat[:1], vec], weighted, what='one matrix')
            check_backward(dev, dn, M, S.sym_solve, dense_solve(M), [mat, vec[:1]], weighted, what='one vector')
            check_backward(dev, dn, M, S.sym_matvec, dense_matvec(M, 0), [mat[:1], vec], weighted,
                           what='matvec one matrix')
        assert mat[:1].shape == (1, K)


@pytest.mark.parametrize('M', [3, 6, 9, 16])
def test_solve_backward_computed_in_float64_on_float32_leaves(dev, M):
    """dtype=torch.float64: float64 result, float32 gradients, held to the float32 bar"""
    S = N().sym
    for n in sizes(M):
        mat, vec, _ = inputs(n, M, 'f32', 300 * M + n)
        md = torch.from_numpy(mat).to(dev).requires_grad_()
        assert S.sym_solve(md, torch.from_numpy(vec).to(dev), dtype=torch.float64).dtype == torch.float64
        for weighted in (True, False):
            check_backward(dev, 'f32', M, lambda m, v: S.sym_solve(m, v, dtype=torch.float64).float(),
                           dense_solve(M), [mat, vec], weighted, what='dtype=')
            check_backward(dev, 'f32', M, lambda m, v: S.sym_solve(m, v, eps=0.125, dtype=torch.float64).float(),
                           dense_solve(M, eps=0.125), [mat[:1], vec], weighted, what='dtype= eps one matrix')


# =========================================================================== sym_invert / sym_det
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16])
def test_invert_and_det_backward(dev, dn, M):
    S = N().sym
    for n in sizes(M):
        mat, _, _ = inputs(n, M, dn, 400 * M + n)
        for weighted in (True, False):
            check_backward(dev, dn, M, S.sym_invert, lambda m: compact(torch.linalg.inv(to_full(m, M))), [mat],
                           weighted, what='sym_invert')
            check_backward(dev, dn, M, lambda m: S.sym_invert(m, diag=True),
                           lambda m: torch.linalg.inv(to_full(m, M)).diagonal(dim1=-2, dim2=-1), [mat],
                           weighted, what='sym_invert diag')
            check_backward(dev, dn, M, S.sym_det, lambda m: torch.linalg.det(to_full(m, M)), [mat], weighted,
                           what='sym_det')


# =========================================================================== batched
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16])
def test_batched_backward(dev, dn, n):
    Bm = N().batched
    for nb in sizes(n):
        rng = np.random.default_rng(500 * n + nb)
        a = (rng.standard_normal((nb, n, n)) + 8 * np.eye(n)).astype(R.NP[dn])
        v = rng.standard_normal((nb, n)).astype(R.NP[dn])
        for weighted in (True, False):
            check_backward(dev, dn, n, Bm.batchinv, torch.linalg.inv, [a], weighted, what='batchinv')
            check_backward(dev, dn, n, Bm.batchdet, torch.linalg.det, [a], weighted, what='batchdet')
            check_backward(dev, dn, n, Bm.batchmatvec, lambda m, x: (m @ x.unsqueeze(-1)).squeeze(-1), [a, v],
                           weighted, what='batchmatvec')
            # a transposed view of the matrix, and a rectangular 3 x 5 one
            check_backward(dev, dn, n, lambda m, x: Bm.batchmatvec(m.transpose(-1, -2), x),
                           lambda m, x: (m.transpose(-1, -2) @ x.unsqueeze(-1)).squeeze(-1), [a, v], weighted,
                           what='batchmatvec transposed')
        if n == 5:
            r = rng.standard_normal((nb, 3, 5)).astype(R.NP[dn])
            for weighted in (True, False):
                check_backward(dev, dn, 5, Bm.batchmatvec, lambda m, x: (m @ x.unsqueeze(-1)).squeeze(-1), [r, v],
                               weighted, what='batchmatvec 3x5')


# =========================================================================== sym_outer / sym_to_full / sym_matmul
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', R.ORDERS)
def test_outer_and_to_full_backward(dev, dn, M):
    S = N().sym
    mat, vec, _ = inputs(N197, M, dn, 600 * M)
    for weighted in (True, False):
        check_backward(dev, dn, M, S.sym_to_full, lambda m: to_full(m, M), [mat], weighted, what='sym_to_full')
        check_backward(dev, dn, M, S.sym_outer, lambda x: compact(x.unsqueeze(-1) * x.unsqueeze(-2)), [vec],
                       weighted, what='sym_outer')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('kd', [(k, d) for k in (2, 3, 4) for d in (2, 3, 4)] + [(5, 3), (3, 6)])
def test_matmul_backward(dev, dn, kd):
    k, d = kd
    S = N().sym
    for diag in (False, True):
        j, h = R.matmul_inputs(N197, k, d, dn, diag)

        def dense(jj, hh):
            Hf = torch.diag_embed(hh) if diag else to_full(hh, k)
            if R.matmul_flips(k, d, diag):
                return compact(jj @ Hf @ jj.transpose(-1, -2))
            return compact(jj.transpose(-1, -2) @ Hf @ jj)
        for weighted in (True, False):
            check_backward(dev, dn, max(k, d), S.sym_matmul, dense, [j, h], weighted, what=f'sym_matmul {diag}')
            # one hessian for every jacobian: its gradient is summed over the batch
            check_backward(dev, dn, max(k, d), S.sym_matmul, dense, [j, h[:1]], weighted, what='one hessian')


# =========================================================================== eig_sym
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('arithmetic', ['reference', 'fast'])
@pytest.mark.parametrize('n', [2, 3, 4, 6])
def test_eig_sym_backward(dev, dn, arithmetic, n):
    """the order- and sign-invariant losses of test_gpu_autograd.py::test_eig_sym_backward; spectra with gaps
    >= 0.1, so that F = 1 / (d_j - d_i) has a usable float32 reference"""
    a, _ = R.eig_inputs(N197, n, 600 + n)
    a = a.astype(R.NP[dn])
    assert R.eig_gap(a) >= R.EIG_GAP * (1 - 1e-5)
    C = np.random.default_rng(n).standard_normal((N197, n, n))
    C = ((C + C.transpose(0, 2, 1)) / 2).astype(R.NP[dn])

    def loss_vals(lam):
        return lam.exp() + lam ** 3

    def loss_full(lam, U, Cm):
        return ((U * torch.tanh(lam).unsqueeze(-2)) @ U.transpose(-1, -2) * Cm).sum((-1, -2)) + loss_vals(lam).sum(-1)

    def sym(x):
        return (x + x.transpose(-1, -2)) / 2
    check_backward(dev, dn, n, lambda x: loss_vals(N().eig_sym(sym(x), arithmetic=arithmetic)),
                   lambda x: loss_vals(torch.linalg.eigvalsh(sym(x))), [a], weighted=False, what='eigenvalues')

    def gpu_full(x):
        lam, U = N().eig_sym(sym(x), compute_u=True, arithmetic=arithmetic)
        return loss_full(lam, U, torch.from_numpy(C).to(dev))

    def dense_full(x):
        lam, U = torch.linalg.eigh(sym(x))
        return loss_full(lam, U, torch.from_numpy(C).to(x.dtype))
    check_backward(dev, dn, n, gpu_full, dense_full, [a], weighted=False, what='eigenvectors')
    check_backward(dev, dn, n, gpu_full, dense_full, [a], weighted=True, what='eigenvectors, weighted')


# =========================================================================== pivoting= with gradients
def definite_and_indefinite(M, dn):
    from test_gpu_large_orders import sym_indefinite_np
    mat, vec = R.spd_np(N197, M, R.NP[dn], 700 + M)
    imat, ivec, idx = sym_indefinite_np(N197, M, R.NP[dn], 800 + M, every=3)
    assert len(idx) > 60
    return (('definite', mat, vec), ('indefinite', imat, ivec))


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', [9, 16])
def test_pivoting_is_validated_with_gradients(dev, dn, M):
    S = N().sym
    mat, vec = R.spd_np(N197, M, R.NP[dn], 700 + M)
    md, vd = torch.from_numpy(mat).to(dev), torch.from_numpy(vec).to(dev)
    for m, v in ((md.clone().requires_grad_(), vd), (md, vd.clone().requires_grad_())):
        with pytest.raises(ValueError, match='pivoting'):
            S.sym_solve(m, v, pivoting='never')
    with pytest.raises(ValueError, match='pivoting'):
        S.sym_invert(md.clone().requires_grad_(), pivoting='never')
    with pytest.raises(ValueError, match='pivoting'):
        S.sym_invert(md.clone().requires_grad_(), diag=True, pivoting='never')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', [9, 16])
def test_pivoting_reaches_forward_and_backward(dev, dn, M, monkeypatch):
    """'always' runs the pivoted kernels in the forward AND in the backward solve; 'always' and 'auto' give the same
    gradients to 4 TOL, on a definite and on an indefinite batch"""
    from nitorch_fastmath_amd import sym as S, _lib
    seen = []
    real = S.launch

    def spy(fn, dev_, dtype, scalars, b, *args, **kw):
        seen.append((getattr(fn, '__name__', ''), scalars))
        return real(fn, dev_, dtype, scalars, b, *args, **kw)
    monkeypatch.setattr(S, 'launch', spy)
    for name, mat, vec in definite_and_indefinite(M, dn):
        w = torch.from_numpy(np.random.default_rng(M).standard_normal(vec.shape).astype(R.NP[dn])).to(dev)
        wk = torch.from_numpy(np.random.default_rng(M + 1).standard_normal(mat.shape).astype(R.NP[dn])).to(dev)
        grads = {}
        for mode in ('auto', 'always'):
            md = torch.from_numpy(mat).to(dev).requires_grad_()
            vd = torch.from_numpy(vec).to(dev).requires_grad_()
            del seen[:]
            x = S.sym_solve(md, vd, pivoting=mode)
            (x * w).sum().backward()
            flags = [s[1] & _lib.MAT_PIVOTED for name_, s in seen if name_ == 'nfm_sym_solve']
            assert len(flags) == 2 and all(bool(f) == (mode == 'always') for f in flags), (mode, seen)
            gm, gv = md.grad.clone(), vd.grad.clone()
            md.grad = None
            del seen[:]
            (S.sym_invert(md, pivoting=mode) * wk).sum().backward()
            flags = [s[1] & _lib.INVERT_PIVOTED for name_, s in seen if name_ == 'nfm_sym_invert']
            assert len(flags) == 1 and bool(flags[0]) == (mode == 'always'), (mode, seen)
            gi = md.grad.clone()
            md.grad = None
            (S.sym_invert(md, diag=True, pivoting=mode) * w).sum().backward()
            grads[mode] = [t_.cpu().numpy() for t_ in (x.detach(), gm, gv, gi, md.grad)]
        for k, (a, b) in enumerate(zip(grads['auto'], grads['always'])):
            assert np.isfinite(a).all() and np.isfinite(b).all()
            print(f'{name} M={M} {dn} result {k}: auto vs always {relerr(a, b):.3g}')
            assert relerr(a, b) <= 4 * TOL[dn], (name, k, relerr(a, b))
