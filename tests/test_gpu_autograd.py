"""Autograd through the HIP kernels, checked against torch's own autograd of dense fp64
equivalents on the CPU (independent implementation)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def N():
    import nitorch_fastmath_amd as N_
    return N_


def to_full(c, M):
    """differentiable compact -> full in plain torch (CPU reference)"""
    rows = [[None] * M for _ in range(M)]
    k = M
    for i in range(M):
        rows[i][i] = c[..., i]
    for i in range(M):
        for j in range(i + 1, M):
            rows[i][j] = rows[j][i] = c[..., k]
            k += 1
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def spd(n, M, seed):
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(n, M, M, dtype=torch.float64, generator=g)
    A = G @ G.transpose(-1, -2) / M + torch.eye(M, dtype=torch.float64)
    cols = [A[:, i, i] for i in range(M)] + [A[:, i, j] for i in range(M) for j in range(i + 1, M)]
    return torch.stack(cols, -1), torch.randn(n, M, dtype=torch.float64, generator=g), torch.randn(n, M, dtype=torch.float64, generator=g)


@pytest.mark.parametrize('M', [2, 3, 4, 6, 12])
def test_sym_solve_and_matvec_backward(dev, M):
    n = 50
    mat, vec, w = spd(n, M, M)
    # CPU reference
    mc, vc = mat.clone().requires_grad_(), vec.clone().requires_grad_()
    x = torch.linalg.solve(to_full(mc, M), vc.unsqueeze(-1)).squeeze(-1)
    (x * w).sum().backward()
    md, vd = mat.to(dev).requires_grad_(), vec.to(dev).requires_grad_()
    xd = N().sym_solve(md, vd)
    assert xd.requires_grad
    (xd * w.to(dev)).sum().backward()
    assert torch.allclose(xd.detach().cpu(), x.detach(), rtol=1e-10, atol=1e-12)
    assert torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-9, atol=1e-11)
    # matvec / addmatvec / submatvec
    for mode, fn in ((0, N().sym_matvec), (1, N().sym_addmatvec), (-1, N().sym_submatvec)):
        mc, vc, ic = mat.clone().requires_grad_(), vec.clone().requires_grad_(), w.clone().requires_grad_()
        y = (to_full(mc, M) @ vc.unsqueeze(-1)).squeeze(-1)
        y = y if mode == 0 else ic + mode * y
        (y * y).sum().backward()
        md, vd, idd = mat.to(dev).requires_grad_(), vec.to(dev).requires_grad_(), w.to(dev).requires_grad_()
        yd = fn(md, vd) if mode == 0 else fn(idd, md, vd)
        (yd * yd).sum().backward()
        assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-9, atol=1e-11)
        assert torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-9, atol=1e-11)
        if mode:
            assert torch.allclose(idd.grad.cpu(), ic.grad, rtol=1e-9, atol=1e-11)


def test_sym_solve_backward_broadcast_and_kinds(dev):
    M, n = 3, 20
    mat, vec, w = spd(n, M, 9)
    # one matrix broadcast against many vectors: the matrix gradient is summed over the batch
    mc, vc = mat[:1].clone().requires_grad_(), vec.clone().requires_grad_()
    x = torch.linalg.solve(to_full(mc, M).expand(n, M, M), vc.unsqueeze(-1)).squeeze(-1)
    (x * w).sum().backward()
    md, vd = mat[:1].to(dev).requires_grad_(), vec.to(dev).requires_grad_()
    (N().sym_solve(md, vd) * w.to(dev)).sum().backward()
    assert md.grad.shape == (1, 6)
    assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-9, atol=1e-11)
    # diagonal and full matrix kinds
    dc, vc = mat[:, :M].clone().requires_grad_(), vec.clone().requires_grad_()
    ((vc / dc) * w).sum().backward()
    dd, vd = mat[:, :M].to(dev).contiguous().requires_grad_(), vec.to(dev).requires_grad_()
    (N().sym_solve(dd, vd) * w.to(dev)).sum().backward()
    assert torch.allclose(dd.grad.cpu(), dc.grad, rtol=1e-9) and torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-9)
    g = torch.Generator().manual_seed(1)
    F = torch.randn(n, M, M, dtype=torch.float64, generator=g) + 4 * torch.eye(M, dtype=torch.float64)
    fc, vc = F.clone().requires_grad_(), vec.clone().requires_grad_()
    (torch.linalg.solve(fc, vc.unsqueeze(-1)).squeeze(-1) * w).sum().backward()
    fd, vd = F.reshape(n, M * M).to(dev).requires_grad_(), vec.to(dev).requires_grad_()
    (N().sym_solve(fd, vd) * w.to(dev)).sum().backward()
    assert torch.allclose(fd.grad.cpu().reshape(n, M, M), fc.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-9, atol=1e-11)
    with pytest.raises(RuntimeError, match='out='):
        N().sym_solve(md, vd, out=torch.empty(n, M, dtype=torch.float64, device=dev))
    with pytest.raises(NotImplementedError):
        N().qr.householder(vd)     # still forward-only


@pytest.mark.parametrize('n', [2, 3, 4, 6])
def test_eig_sym_backward(dev, n):
    nb = 30
    g = torch.Generator().manual_seed(n)
    a = torch.randn(nb, n, n, dtype=torch.float64, generator=g)
    a = (a + a.transpose(-1, -2)) / 2
    C = torch.randn(nb, n, n, dtype=torch.float64, generator=g)
    C = (C + C.transpose(-1, -2)) / 2

    def loss_vals(lam):
        return (lam.exp() + lam ** 3).sum()       # symmetric in the eigenvalues: order-free

    def loss_full(lam, U):                          # order- and sign-invariant
        return ((U * torch.tanh(lam).unsqueeze(-2)) @ U.transpose(-1, -2) * C).sum() + loss_vals(lam)

    ac = a.clone().requires_grad_()
    lam, U = torch.linalg.eigh((ac + ac.transpose(-1, -2)) / 2)
    loss_vals(lam).backward()
    g_vals = ac.grad.clone()
    ac.grad = None
    lam, U = torch.linalg.eigh((ac + ac.transpose(-1, -2)) / 2)
    loss_full(lam, U).backward()
    g_full = ac.grad.clone()

    ad = a.to(dev).requires_grad_()
    lam_d = N().eig_sym((ad + ad.transpose(-1, -2)) / 2)
    loss_vals(lam_d).backward()
    assert torch.allclose(ad.grad.cpu(), g_vals, rtol=1e-8, atol=1e-9)
    ad.grad = None
    lam_d, U_d = N().eig_sym((ad + ad.transpose(-1, -2)) / 2, compute_u=True)
    Cd = C.to(dev)
    (((U_d * torch.tanh(lam_d).unsqueeze(-2)) @ U_d.transpose(-1, -2) * Cd).sum() + loss_vals(lam_d)).backward()
    assert torch.allclose(ad.grad.cpu(), g_full, rtol=1e-7, atol=1e-8)


def test_reduce_backward(dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 33, 7, dtype=torch.float64, generator=g)
    x[torch.rand(x.shape, generator=g) < 0.1] = float('nan')
    w = torch.randn(5, 7, dtype=torch.float64, generator=g)
    R = N().reduce
    for ours, ref, dim in ((R.nansum, torch.nansum, 1), (R.nanmean, torch.nanmean, 1), (R.nansum, torch.nansum, None),
                           (R.nanmean, torch.nanmean, (0, 2))):
        xc = x.clone().requires_grad_()
        xd = x.to(dev).requires_grad_()
        if dim is None:
            (ref(xc) * 3).backward()
            (ours(xd) * 3).backward()
        elif dim == 1:
            (ref(xc, dim=dim) * w).sum().backward()
            (ours(xd, dim=dim) * w.to(dev)).sum().backward()
        else:
            v = torch.arange(33, dtype=torch.float64)
            (ref(xc, dim=dim) * v).sum().backward()
            (ours(xd, dim=dim) * v.to(dev)).sum().backward()
        assert torch.equal(torch.isnan(xd.grad.cpu()), torch.isnan(xc.grad))
        assert torch.allclose(torch.nan_to_num(xd.grad.cpu()), torch.nan_to_num(xc.grad), rtol=1e-12, atol=1e-14)
    y = torch.randn(4, 9, dtype=torch.float64, generator=g)
    yc, yd = y.clone().requires_grad_(), y.to(dev).requires_grad_()
    (torch.sum(yc, 1) ** 2).sum().backward()
    (R.sum(yd, 1, keepdim=True) ** 2).sum().backward()
    assert torch.allclose(yd.grad.cpu(), yc.grad)
    yc.grad = None; yd.grad = None
    torch.mean(yc).backward()
    R.mean(yd).backward()
    assert torch.allclose(yd.grad.cpu(), yc.grad)
    with pytest.raises(NotImplementedError):
        R.median(yd, dim=1) if False else N().qr.hessenberg(torch.randn(3, 3, device=dev, requires_grad=True))


@pytest.mark.parametrize('n', [1, 2, 3, 4, 6])
def test_batched_backward(dev, n):
    """batchmatvec / batchinv / batchdet against torch's autograd of the dense fp64 ops on the CPU"""
    g = torch.Generator().manual_seed(n)
    a = torch.randn(7, n, n, dtype=torch.float64, generator=g) + 4 * torch.eye(n, dtype=torch.float64)
    v = torch.randn(7, n, dtype=torch.float64, generator=g)
    w = torch.randn(7, n, n, dtype=torch.float64, generator=g)
    B = N().batched
    ac, vc = a.clone().requires_grad_(), v.clone().requires_grad_()
    ad, vd = a.to(dev).requires_grad_(), v.to(dev).requires_grad_()
    (torch.matmul(ac, vc.unsqueeze(-1)).squeeze(-1) * w[:, 0]).sum().backward()
    (B.batchmatvec(ad, vd) * w[:, 0].to(dev)).sum().backward()
    assert torch.allclose(ad.grad.cpu(), ac.grad, rtol=1e-11, atol=1e-12)
    assert torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-11, atol=1e-12)
    # broadcast vector: one vector for every matrix
    v1c, v1d = v[0].clone().requires_grad_(), v[0].to(dev).requires_grad_()
    (torch.matmul(a, v1c) * w[:, 0]).sum().backward()
    (B.batchmatvec(a.to(dev), v1d) * w[:, 0].to(dev)).sum().backward()
    assert torch.allclose(v1d.grad.cpu(), v1c.grad, rtol=1e-11, atol=1e-12)
    for ours, ref, wt in ((B.batchinv, torch.linalg.inv, w), (B.batchdet, torch.linalg.det, w[:, 0, 0])):
        ac, ad = a.clone().requires_grad_(), a.to(dev).requires_grad_()
        (ref(ac) * wt).sum().backward()
        (ours(ad) * wt.to(dev)).sum().backward()
        assert torch.allclose(ad.grad.cpu(), ac.grad, rtol=1e-9, atol=1e-10), ours.__name__


@pytest.mark.parametrize('M', [1, 2, 3, 4, 6])
def test_sym_invert_and_det_backward(dev, M):
    mat, v, w = spd(9, M, 40 + M)
    S = N().sym
    K = M * (M + 1) // 2
    wk = torch.randn(9, K, dtype=torch.float64, generator=torch.Generator().manual_seed(M))

    def compact(full):
        cols = [full[..., i, i] for i in range(M)] + [full[..., i, j] for i in range(M) for j in range(i + 1, M)]
        return torch.stack(cols, -1)
    mc, md = mat.clone().requires_grad_(), mat.to(dev).requires_grad_()
    (compact(torch.linalg.inv(to_full(mc, M))) * wk).sum().backward()
    (S.sym_invert(md) * wk.to(dev)).sum().backward()
    assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-9, atol=1e-10)
    mc, md = mat.clone().requires_grad_(), mat.to(dev).requires_grad_()
    (torch.linalg.inv(to_full(mc, M)).diagonal(dim1=-2, dim2=-1) * w).sum().backward()
    (S.sym_invert(md, diag=True) * w.to(dev)).sum().backward()
    assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-9, atol=1e-10)
    mc, md = mat.clone().requires_grad_(), mat.to(dev).requires_grad_()
    (torch.linalg.det(to_full(mc, M)) * w[:, 0]).sum().backward()
    (S.sym_det(md) * w[:, 0].to(dev)).sum().backward()
    assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-9, atol=1e-10)


def test_pick_and_var_backward(dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 9, 5, dtype=torch.float64, generator=g)
    R = N().reduce
    w = torch.randn(4, 5, dtype=torch.float64, generator=g)
    for name, ref in (('max', lambda t: t.amax(1)), ('min', lambda t: t.amin(1))):
        xc, xd = x.clone().requires_grad_(), x.to(dev).requires_grad_()
        (ref(xc) * w).sum().backward()
        (getattr(R, name)(xd, dim=1) * w.to(dev)).sum().backward()
        assert torch.equal(xd.grad.cpu(), xc.grad), name
        xc, xd = x.clone().requires_grad_(), x.to(dev).requires_grad_()
        ref(xc).sum().backward()
        val, idx = getattr(R, name)(xd, dim=1, keepdim=True, return_indices=True)
        val.sum().backward()
        assert val.shape == (4, 1, 5) and torch.equal(xd.grad.cpu(), xc.grad)
    # several dims, NaNs skipped, full reduction
    xn = x.clone()
    xn[torch.rand(xn.shape, generator=g) < 0.2] = float('nan')
    xc, xd = xn.clone().requires_grad_(), xn.to(dev).requires_grad_()
    torch.nan_to_num(xc, nan=-float('inf')).amax((0, 2)).sum().backward()
    R.nanmax(xd, dim=(0, 2)).sum().backward()
    assert torch.equal(xd.grad.cpu(), xc.grad)
    xc, xd = x.clone().requires_grad_(), x.to(dev).requires_grad_()
    (xc.max() * 2).backward()
    (R.max(xd) * 2).backward()
    assert torch.equal(xd.grad.cpu(), xc.grad)
    # var / std, biased and unbiased, one and several dims
    for dim in (1, (0, 2), None):
        for unb in (True, False):
            for ours, ref in ((R.var, torch.var), (R.std, torch.std)):
                xc, xd = x.clone().requires_grad_(), x.to(dev).requires_grad_()
                kw = {} if dim is None else {'dim': dim}
                r = ref(xc, unbiased=unb, **kw)
                o = ours(xd, dim=dim, unbiased=unb)
                assert torch.allclose(o.detach().cpu(), r.detach(), rtol=1e-12)
                (r ** 2).sum().backward()
                (o ** 2).sum().backward()
                assert torch.allclose(xd.grad.cpu(), xc.grad, rtol=1e-10, atol=1e-12), (dim, unb, ours.__name__)
    # nanvar: gradient only on the counted elements
    xd = xn.to(dev).requires_grad_()
    R.nanvar(xd, dim=1).sum().backward()
    mask = (~torch.isnan(xn)).double()
    xc = torch.nan_to_num(xn).requires_grad_()           # NaN-free leaf: masked arithmetic instead
    cnt = mask.sum(1, keepdim=True)
    mean = (xc * mask).sum(1, keepdim=True) / cnt
    ((((xc - mean) ** 2) * mask).sum(1) / (cnt.squeeze(1) - 1)).sum().backward()
    assert torch.allclose(xd.grad.cpu(), xc.grad * mask, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('M', [1, 2, 3, 4, 5])
def test_sym_to_full_outer_matmul_backward(dev, M):
    mat, v, w = spd(6, M, 70 + M)
    S = N().sym
    g = torch.Generator().manual_seed(M)
    wf = torch.randn(6, M, M, dtype=torch.float64, generator=g)
    K = M * (M + 1) // 2
    wk = torch.randn(6, K, dtype=torch.float64, generator=g)

    def compact(full, n):
        cols = [full[..., i, i] for i in range(n)] + [full[..., i, j] for i in range(n) for j in range(i + 1, n)]
        return torch.stack(cols, -1)
    mc, md = mat.clone().requires_grad_(), mat.to(dev).requires_grad_()
    (to_full(mc, M) * wf).sum().backward()
    (S.sym_to_full(md) * wf.to(dev)).sum().backward()
    assert torch.allclose(md.grad.cpu(), mc.grad, rtol=1e-12, atol=1e-13)
    vc, vd = v.clone().requires_grad_(), v.to(dev).requires_grad_()
    (compact(vc.unsqueeze(-1) * vc.unsqueeze(-2), M) * wk).sum().backward()
    (S.sym_outer(vd) * wk.to(dev)).sum().backward()
    assert torch.allclose(vd.grad.cpu(), vc.grad, rtol=1e-12, atol=1e-13)
    for d in (1, 2, 3, 4):
        if M > 4:
            continue
        J = torch.randn(6, M, d, dtype=torch.float64, generator=g)
        Kd = d * (d + 1) // 2
        wd = torch.randn(6, Kd, dtype=torch.float64, generator=g)
        flip = M == d and M in (2, 3)                        # quirk Q16: the reference computes J H J^T
        jc, hc = J.clone().requires_grad_(), mat.clone().requires_grad_()
        jd, hd = J.to(dev).requires_grad_(), mat.to(dev).requires_grad_()
        Hf = to_full(hc, M)
        full = jc @ Hf @ jc.transpose(-1, -2) if flip else jc.transpose(-1, -2) @ Hf @ jc
        (compact(full, d) * wd).sum().backward()
        out = S.sym_matmul(jd, hd)
        assert torch.allclose(out.detach().cpu(), compact(full, d).detach(), rtol=1e-12, atol=1e-12)
        (out * wd.to(dev)).sum().backward()
        assert torch.allclose(jd.grad.cpu(), jc.grad, rtol=1e-10, atol=1e-11), (M, d)
        assert torch.allclose(hd.grad.cpu(), hc.grad, rtol=1e-10, atol=1e-11), (M, d)
        # diagonal hessian, one hessian for every jacobian (broadcast)
        dc, dd = mat[0, :M].clone().requires_grad_(), mat[0, :M].to(dev).requires_grad_()
        jc, jd = J.clone().requires_grad_(), J.to(dev).requires_grad_()
        (compact(jc.transpose(-1, -2) @ torch.diag_embed(dc) @ jc, d) * wd).sum().backward()
        (S.sym_matmul(jd, dd) * wd.to(dev)).sum().backward()
        if M > 1:       # (M == 1: a 1-vector is read as compact 1x1, same thing)
            assert torch.allclose(dd.grad.cpu(), dc.grad, rtol=1e-10, atol=1e-11), (M, d)
        assert torch.allclose(jd.grad.cpu(), jc.grad, rtol=1e-10, atol=1e-11), (M, d)


def test_median_backward(dev):
    """the gradient of a median goes to the element that was picked (what torch.median's own
    backward does on the reference's path)"""
    import nitorch_fastmath_amd as N_
    torch.manual_seed(4)
    x = torch.randn(6, 9, 5, device=dev, dtype=torch.float64, requires_grad=True)
    v, i = N_.reduce.median(x, dim=1, return_indices=True)
    v.sum().backward()
    ref = torch.zeros_like(x)
    ref.scatter_(1, i.unsqueeze(1), 1.0)
    assert torch.equal(x.grad, ref) and x.grad.sum() == 30
    xr = x.detach().clone().requires_grad_(True)
    torch.median(xr, dim=1).values.sum().backward()
    assert torch.equal(x.grad, xr.grad)                     # no duplicates in a random draw: same element
    y = torch.randn(1000, device=dev, requires_grad=True)
    N_.reduce.median(y).backward()
    assert y.grad.sum() == 1 and y.grad[y.detach().argsort()[499]] == 1


# ---------------------------------------------------------------------------------------------------------------
# Gradients of `reduce` on every route: float32 and float64 leaves, scalar / negative / adjacent / non-adjacent
# (staged) / unsorted dims and the full reduction, keepdim both ways, dtype=, views, long reduced axes.
# Expected gradients are the closed forms of tests/_reduce_ref.py in longdouble:
#     sum   g on the counted elements (0 at omitted NaNs)      mean  g / n
#     var   2 (x - mean) g / (n - ddof)                        std   var's gradient / (2 std)
#     max, min, median   the whole cotangent at the returned index (first occurrence)
# Bound per entry: eps |ref| (eps of the leaf's dtype) + the forward error propagated to first order,
#     var   2 |g| / (n - ddof) . (eps64 |mean| + 2 n u R)
#     std   that / (2 std) + |ref| (eps64 std + 8 n u R^2 n / ((n - ddof) 2 std)) / std
# (the mean / variance terms of _reduce_ref.py, u = 2^-53, R = max - min of the slice).
_GDT = {'f32': torch.float32, 'f64': torch.float64}
_GRAD_DIMS = (1, -1, (1, 2), (0, 3), (2, 1), None)       # (0, 3): staged; (2, 1): unsorted


def _leaf(x, dev, view=None):
    """leaf on the device (and the tensor the function sees: the leaf itself or a view of it)"""
    leaf = torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_()
    return leaf, (leaf if view is None else view(leaf))


def _cotangent(out, rng, dev):
    g = rng.standard_normal(tuple(out.shape))
    gt = torch.from_numpy(g).to(out.dtype)
    return gt.double().numpy(), gt.to(dev)


def _grad_data(shape, dn, seed, nan_rate=0.05):
    rng = np.random.default_rng(seed)
    x = (3.0 + rng.standard_normal(shape)).astype(np.float32 if dn == 'f32' else np.float64)
    if nan_rate:
        x[rng.random(shape) < nan_rate] = np.nan
    return x, rng


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('omitnan', [True, False])
def test_reduce_gradients_every_dim(dev, dn, omitnan):
    import _reduce_ref as RR
    R = N().reduce
    x, rng = _grad_data((5, 70, 6, 33), dn, 31, 0.05 if omitnan else 0.0)
    if not omitnan:
        x[1, 5, 2, 7] = np.nan                         # one NaN: var / std propagate it to their slices' gradients
    worst = 0.0
    for di, dim in enumerate(_GRAD_DIMS):
        tr = RR.Truth(x, dim)
        # keepdim both ways on the scalar and the staged dims, alternating elsewhere; dtype=float64 with keepdim
        for keepdim in ((False, True) if dim in (1, (0, 3)) else (bool(di % 2),)):
            for fn, ddof in (('sum', 0), ('mean', 0), ('var', 1), ('var', 0), ('std', 1), ('std', 0)):
                for odt in ((None, torch.float64) if dn == 'f32' and keepdim else (None,)):
                    leaf, xin = _leaf(x, dev)
                    kw = {} if fn in ('sum', 'mean') else {'unbiased': bool(ddof)}
                    out = getattr(R, fn)(xin, dim, keepdim, omitnan=omitnan, dtype=odt, **kw)
                    assert out.dtype == (odt or _GDT[dn])
                    g, gd = _cotangent(out, rng, dev)
                    (out * gd).sum().backward()
                    assert leaf.grad.dtype == _GDT[dn]
                    ref, bound = RR.grad_truth(x, dim, fn, g, ddof, omitnan, tr)
                    what = (fn, ddof, dim, keepdim, odt)
                    worst = max(worst, RR.judge_grad(leaf.grad.cpu().numpy(), ref, bound, what))
                    if omitnan:                        # exactly zero at the omitted positions
                        assert (leaf.grad.cpu().numpy()[np.isnan(x)] == 0).all(), what
    print(f'GRAD {dn} omitnan={omitnan}: worst error/bound {worst:.3g}')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_reduce_gradients_long_axes_and_counts(dev, dn):
    """reduced lengths that put the forward pass and RED_NANCOUNT on a chunked plan ((3, 70_001): FLAT, 68 chunks;
    (2, 1025, 3): FLAT, 3 chunks), and the counts of every dim choice, compared exactly"""
    import _reduce_ref as RR
    from nitorch_fastmath_amd import _lib
    R = N().reduce
    for shape, dims in (((3, 70_001), (1, None)), ((2, 1025, 3), (1, (0, 1))), ((5, 70, 6, 33), _GRAD_DIMS)):
        x, rng = _grad_data(shape, dn, 37 + len(shape))
        xd = torch.from_numpy(x).to(dev)
        for dim in dims:
            cnt = R._reduce(_lib.RED_NANCOUNT, xd, dim, True, torch.float64)[0].cpu().numpy()
            ax = None if dim is None else (tuple(dim) if isinstance(dim, tuple) else dim)
            assert np.array_equal(cnt, (~np.isnan(x)).sum(axis=ax, keepdims=True).astype(np.float64)), (shape, dim)
        if len(shape) == 4:
            continue
        for dim in dims:
            for fn, ddof in (('sum', 0), ('mean', 0), ('var', 1), ('std', 0)):
                leaf, xin = _leaf(x, dev)
                kw = {} if fn in ('sum', 'mean') else {'unbiased': bool(ddof)}
                out = getattr(R, fn)(xin, dim, omitnan=True, **kw)
                g, gd = _cotangent(out, rng, dev)
                (out * gd).sum().backward()
                ref, bound = RR.grad_truth(x, dim, fn, g, ddof, True)
                RR.judge_grad(leaf.grad.cpu().numpy(), ref, bound, (shape, fn, dim))
            for which in ('max', 'min'):
                leaf, xin = _leaf(x, dev)
                out = getattr(R, which)(xin, dim, omitnan=True)
                g, gd = _cotangent(out, rng, dev)
                (out * gd).sum().backward()
                ref, _ = RR.pick_truth(x, dim, which, g, True)
                assert np.array_equal(leaf.grad.cpu().numpy().astype(np.longdouble), ref), (shape, which, dim)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_reduce_gradients_through_views(dev, dn):
    """a permuted view (reduced in place through the mapped dims) and a strided slice as input: the gradient
    arrives in the leaf's own layout"""
    import _reduce_ref as RR
    R = N().reduce
    base, rng = _grad_data((2, 6, 7, 9, 5), dn, 41)
    views = ((lambda t: t.permute(0, 2, 3, 4, 1), lambda a: a.transpose(0, 2, 3, 4, 1), (-1, (1, 2), (0, 4))),
             (lambda t: t[:, 1::2, :, ::3], lambda a: a[:, 1::2, :, ::3], (1, (2, 3), None)))
    for tview, nview, dims in views:
        xv = nview(base)
        for dim in dims:
            for fn, ddof in (('sum', 0), ('mean', 0), ('var', 1), ('std', 1)):
                leaf, xin = _leaf(base, dev, tview)
                assert not xin.is_contiguous()
                kw = {} if fn in ('sum', 'mean') else {'unbiased': bool(ddof)}
                out = getattr(R, fn)(xin, dim, omitnan=True, **kw)
                g, gd = _cotangent(out, rng, dev)
                (out * gd).sum().backward()
                ref, bound = RR.grad_truth(xv, dim, fn, g, ddof, True)
                full_ref, full_bound = np.zeros(base.shape, np.longdouble), np.zeros(base.shape, np.longdouble)
                nview(full_ref)[...] = ref                # entries outside the view get no gradient
                nview(full_bound)[...] = bound
                RR.judge_grad(leaf.grad.cpu().numpy(), full_ref, full_bound, (fn, dim))
            for which in ('max', 'min'):
                leaf, xin = _leaf(base, dev, tview)
                out = getattr(R, which)(xin, dim, omitnan=True)
                g, gd = _cotangent(out, rng, dev)
                (out * gd).sum().backward()
                ref, _ = RR.pick_truth(xv, dim, which, g, True)
                full_ref = np.zeros(base.shape, np.longdouble)
                nview(full_ref)[...] = ref
                assert np.array_equal(leaf.grad.cpu().numpy().astype(np.longdouble), full_ref), (which, dim)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_pick_gradients_ties_and_nans(dev, dn):
    """max / min / nanmax / nanmin: the returned index is the first occurrence (numpy's argmax / argmin), it gets the
    whole cotangent; the omitting forms leave NaN positions (an all-NaN slice included) without gradient, the
    propagating forms send the cotangent to the first NaN"""
    import _reduce_ref as RR
    R = N().reduce
    x, rng = _grad_data((5, 70, 6, 33), dn, 43)
    x[rng.random(x.shape) < 0.2] = 4.5                 # ties, above most of the data: often the maximum
    x[rng.random(x.shape) < 0.1] = 0.5                 # and below: often the minimum
    x[2, :, 3, 7] = np.nan                             # an all-NaN slice for dim 1
    for omitnan in (True, False):
        for dim in (1, -1, (1, 2), (0, 3), None):
            for keepdim in (False, True):
                for which in ('max', 'min'):
                    leaf, xin = _leaf(x, dev)
                    if dim is not None and not isinstance(dim, tuple):
                        out, idx = getattr(R, which)(xin, dim, keepdim, omitnan=omitnan, return_indices=True)
                    else:
                        out, idx = getattr(R, which)(xin, dim, keepdim, omitnan=omitnan), None
                    g, gd = _cotangent(out, rng, dev)
                    (out * gd).sum().backward()
                    ref, arg = RR.pick_truth(x, dim, which, g, omitnan)
                    what = (which, omitnan, dim, keepdim)
                    assert np.array_equal(leaf.grad.cpu().numpy().astype(np.longdouble), ref), what
                    if idx is not None:
                        assert np.array_equal(idx.cpu().numpy().reshape(-1), arg), what


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_median_gradients(dev, dn):
    """ties and omitnan=True through the rows kernel, >= 4096 rows of a middle dim through the per-lane kernel,
    a row longer than 1024 (radix selection): the whole cotangent at the returned index, which holds the median"""
    R = N().reduce
    rng = np.random.default_rng(47)
    dt = np.float32 if dn == 'f32' else np.float64
    for shape, dim, omitnan in (((40, 33), 1, True), ((40, 33), 1, False), ((2, 9, 5000), 1, True), ((3, 1500), 1, True),
                                ((3, 1500), 1, False)):
        x = np.round(rng.standard_normal(shape) * 4).astype(dt) / 4 + 0        # a grid of values: many ties (no -0)
        if omitnan:
            x[rng.random(shape) < 0.1] = np.nan
        leaf, xin = _leaf(x, dev)
        out, idx = R.median(xin, dim, omitnan=omitnan, return_indices=True)
        g, gd = _cotangent(out, rng, dev)
        (out * gd).sum().backward()
        xs = np.moveaxis(x, dim, -1)
        srt = np.sort(xs, -1)                                                # NaNs last
        cnt = (~np.isnan(xs)).sum(-1)
        med = np.take_along_axis(srt, ((cnt - 1) // 2)[..., None], -1)[..., 0]     # the lower median
        assert np.array_equal(out.detach().cpu().numpy(), med), (shape, omitnan)
        first = (xs == med[..., None]).argmax(-1)                            # its first occurrence
        assert np.array_equal(idx.cpu().numpy(), first), (shape, omitnan)
        ref = np.zeros(xs.shape)
        np.put_along_axis(ref, first[..., None], g[..., None], -1)
        assert np.array_equal(leaf.grad.cpu().numpy().astype(np.float64), np.moveaxis(ref, -1, dim)), (shape, omitnan)


def test_reduce_gradients_degenerate_slices_and_out(dev):
    """std of a constant slice and var with n = ddof give what torch gives on the CPU (0 where std == 0: torch masks
    the division; NaN for n = ddof), no exception; out= with a leaf that requires grad still raises"""
    R = N().reduce
    x = torch.tensor([[2.0, 2.0, 2.0, 2.0], [1.0, 2.0, 3.0, 5.0]], dtype=torch.float64)
    for ours, ref, kw in ((R.std, torch.std, {}), (R.var, torch.var, {}), (R.std, torch.std, {'unbiased': False})):
        xc, xd = x.clone().requires_grad_(), x.to(dev).requires_grad_()
        ref(xc, dim=1, **kw).sum().backward()
        ours(xd, dim=1, **kw).sum().backward()
        got = xd.grad.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(xc.grad)) and torch.equal(torch.isinf(got), torch.isinf(xc.grad))
        assert torch.allclose(torch.nan_to_num(got, 0, 0, 0), torch.nan_to_num(xc.grad, 0, 0, 0), rtol=1e-13, atol=0)
    one = x[:, :1].contiguous()                          # n = ddof = 1
    xc, xd = one.clone().requires_grad_(), one.to(dev).requires_grad_()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        torch.var(xc, dim=1).sum().backward()
    R.var(xd, dim=1).sum().backward()
    got = xd.grad.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(xc.grad)) and torch.equal(torch.isinf(got), torch.isinf(xc.grad))
    leaf = x.to(dev).requires_grad_()
    for fn in (R.max, R.min, R.median, R.nanmax):
        with pytest.raises(RuntimeError):
            fn(leaf, dim=1, out=torch.empty(2, dtype=torch.float64, device=dev))
