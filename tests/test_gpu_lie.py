"""`lie.expm` / `expm_derivatives` on the MI355X: against the fixture's 40-digit truth and the reference's own
outputs, structure, scale, layouts, non-finite input, streams, derivatives, autograd and the torch route.

Error of a result K against the truth T: max|K - T| / max|T|, per matrix.  The bound everywhere is
C * D * eps * (1 + ||X||_1), with C from profiles/expm_accuracy.md."""
import os
import numpy as np
import pytest
import torch
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

C_EXPM = 4     # profiles/expm_accuracy.md: worst measured C is 0.57 (fixture), see the table for 10^6 random
C_DERIV = 4

DT = {'f32': torch.float32, 'f64': torch.float64}


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLDEN, 'lie.npz'))


@pytest.fixture(scope='module')
def N():
    import nitorch_fastmath_amd as N
    return N


def rel(k, t):
    k, t = np.asarray(k, np.float64), np.asarray(t, np.float64)
    ax = tuple(range(k.ndim - 2, k.ndim))
    return np.abs(k - t).max(ax) / np.abs(t).max(ax)


def bound(x, c, dtype):
    x = np.asarray(x, np.float64)
    n1 = np.abs(x).sum(-2).max(-1)
    return c * x.shape[-1] * torch.finfo(dtype).eps * (1 + n1)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('D', range(1, 9))
def test_golden(N, g, dt, D):
    x, ref, true, cls = (g[f'{k}_{dt}_{D}'] for k in ('x', 'ref', 'true', 'cls'))
    dtype = DT[dt]
    k = N.lie.expm(torch.from_numpy(x).cuda()).cpu().numpy()
    ek, er = rel(k, true), rel(ref, true)
    eps = torch.finfo(dtype).eps
    acc = (cls > 0) & (cls <= 1)            # where the reference is accurate
    assert np.all(ek[acc] <= 2 * er[acc] + 4 * D * eps), (ek[acc].max(), er[acc].max())
    fin = np.isfinite(true).all((1, 2))
    assert np.all(ek[fin] <= bound(x[fin], C_EXPM, dtype)), (ek / bound(x, C_EXPM, dtype)).max()


def test_golden_bases(N, g):
    for name in ('rigid', 'affine'):
        B, p, true = (torch.from_numpy(g[f'{name}_{k}']) for k in ('basis', 'x', 'true'))
        k = N.lie.expm(p.cuda(), B.cuda()).cpu()
        M = torch.einsum('nf,fij->nij', p, B)
        assert np.all(rel(k, true) <= bound(M, C_EXPM, torch.float64))
        assert np.all(rel(k, g[f'{name}_ref']) <= bound(M, C_EXPM, torch.float64))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [2, 3, 4, 6, 8])
def test_structure(N, dtype, D):
    gen = torch.Generator().manual_seed(D)
    eps = torch.finfo(dtype).eps
    I = torch.eye(D, dtype=torch.float64)
    s = torch.randn(500, D, D, dtype=torch.float64, generator=gen)
    s = (s - s.mT) * 2                                    # skew-symmetric: expm is orthogonal
    q = N.lie.expm(s.to(dtype).cuda()).double().cpu()
    assert np.all(rel(q.mT @ q, I.expand_as(q)) <= bound(s, C_EXPM, dtype))
    n = torch.triu(torch.randn(500, D, D, dtype=torch.float64, generator=gen), 1).to(dtype).double()
    fs, t = I.expand_as(n).clone(), I.expand_as(n).clone()
    for k in range(1, D):                                 # nilpotent: the finite sum
        t = t @ n / k
        fs = fs + t
    e = N.lie.expm(n.to(dtype).cuda()).double().cpu()
    assert np.all(rel(e, fs) <= bound(n, C_EXPM, dtype))
    z = N.lie.expm(torch.zeros(7, D, D, dtype=dtype, device='cuda')).cpu()
    assert torch.equal(z, torch.eye(D, dtype=dtype).expand(7, D, D))
    x = torch.randn(500, D, D, dtype=torch.float64, generator=gen)
    x = (x / x.abs().sum(-2).amax(-1)[:, None, None]).to(dtype).cuda()      # ||X||_1 = 1
    pm = (N.lie.expm(x) @ N.lie.expm(-x)).double().cpu()
    assert np.all(rel(pm, I.expand_as(pm)) <= 4 * bound(x.cpu(), C_EXPM, dtype))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [3, 4])
def test_scale(N, dtype, D):
    gen = torch.Generator(device='cuda').manual_seed(7)
    x = (torch.randn(10 ** 6, D, D, dtype=torch.float64, device='cuda', generator=gen) * 0.7).to(dtype)
    k = N.lie.expm(x).double()
    t = torch.linalg.matrix_exp(x.double())
    err = ((k - t).abs().amax((-2, -1)) / t.abs().amax((-2, -1)))
    n1 = x.double().abs().sum(-2).amax(-1)
    # float64: matrix_exp's own error is of the same order, hence twice the bound
    c = C_EXPM if dtype == torch.float32 else 2 * C_EXPM
    assert bool((err <= c * D * torch.finfo(dtype).eps * (1 + n1)).all()), float(err.max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [1, 3, 4, 7])
def test_layouts_bit_for_bit(N, dtype, D):
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(301, D, D + 1, dtype=dtype, generator=gen).cuda()
    f = N.lie.expm
    cases = [base[..., :D].mT, base[::2, :, :D], base[..., :D],                      # transposed, every other, padded
             base[:1, :, :D].expand(5, D, D), base[:, :, :D].reshape(7, 43, D, D),
             base[:1, :, :D], base[:0, :, :D]]
    for v in cases:
        out = f(v)
        assert out.is_contiguous() and out.shape == v.shape
        assert torch.equal(out, f(v.contiguous()))
    for n in (1, 63, 65, 257, 1001):
        x = torch.randn(n, D, D, dtype=dtype, generator=gen).cuda()
        assert torch.equal(f(x)[n // 2], f(x[n // 2:n // 2 + 1])[0])


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_non_finite_input(N, dtype):
    x = torch.randn(6, 4, 4, dtype=dtype) * 0.3
    x[1, 2, 3] = float('nan')
    x[2, 0, 0] = float('inf')
    x[3, 1, 1] = -float('inf')
    x[4] = torch.finfo(dtype).max / 8                  # huge and finite: ends, overflows
    e = N.lie.expm(x.cuda()).cpu()
    assert torch.isnan(e[1:4]).all()
    assert torch.isfinite(e[0]).all() and torch.isfinite(e[5]).all()
    assert torch.equal(e[0], N.lie.expm(x[:1].cuda()).cpu()[0])
    for D in (1, 2, 4):
        xx = torch.full((3, D, D), float('nan'), dtype=dtype).cuda()
        assert torch.isnan(N.lie.expm(xx)).all()
        r = N.lie.expm_derivatives(xx, grad_X=True)[1]
        assert torch.isnan(r).all()


def test_side_stream(N):
    x = torch.randn(5000, 4, 4, device='cuda') * 0.5
    ref = N.lie.expm(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = N.lie.expm(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


@pytest.mark.parametrize('D', [2, 3, 4])
def test_derivatives_golden(N, g, D):
    x = torch.from_numpy(g[f'dx_{D}']).cuda()
    e, dX, dB, hX = N.lie.expm_derivatives(x, grad_X=True, grad_basis=True, hess_X=True)
    F = D * D
    assert dX.shape == (2, F, D, D) and dB.shape == (2, F, D, D, D, D) and hX.shape == (2, F, F, D, D)
    assert all(t.is_contiguous() for t in (e, dX, dB, hX))
    xn = g[f'dx_{D}']
    b = bound(xn, C_DERIV, torch.float64)
    assert np.all(rel(e.cpu(), g[f'dtrue_e_{D}']) <= b)
    scale = lambda a: np.abs(a).reshape(2, -1).max(1)                                    # noqa: E731
    err = lambda k, t: np.abs(np.asarray(k) - t).reshape(2, -1).max(1) / scale(t)        # noqa: E731
    assert np.all(err(dX.cpu(), g[f'dtrue_dX_{D}']) <= b)
    assert np.all(err(hX.cpu(), g[f'dtrue_hX_{D}']) <= b)
    tdB = xn.reshape(2, F, 1, 1, 1, 1) * g[f'dtrue_dX_{D}'].reshape(2, 1, D, D, D, D)
    assert np.all(err(dB.cpu(), tdB) <= b)
    # the reference's own derivatives, matrix by matrix (its hess_X is unbatched only: Q19)
    assert np.all(err(dX.cpu(), g[f'dref_dX_{D}']) <= b + err(g[f'dref_dX_{D}'], g[f'dtrue_dX_{D}']))
    # batched X with hess_X (the reference raises) = the matrices one by one
    h1 = N.lie.expm_derivatives(x[1], hess_X=True)[1]
    assert h1.shape == (F, F, D, D) and torch.allclose(h1, hX[1], rtol=0, atol=0)


@pytest.mark.parametrize('D', [2, 4, 5, 9])
def test_derivatives_with_basis_and_torch_route(N, D):
    gen = torch.Generator().manual_seed(D)
    F = 5
    B = (torch.randn(F, D, D, dtype=torch.float64, generator=gen) * 0.3).cuda()
    p = (torch.randn(3, F, dtype=torch.float64, generator=gen)).cuda()
    e, dX, dB, hX = N.lie.expm_derivatives(p, B, grad_X=True, grad_basis=True, hess_X=True)
    assert e.shape == (3, D, D) and dX.shape == (3, F, D, D) and dB.shape == (3, F, D, D, D, D)
    assert hX.shape == (3, F, F, D, D)
    M = torch.einsum('nf,fij->nij', p, B)
    from torch.func import jvp

    def L(a):
        return jvp(torch.linalg.matrix_exp, (M,), (a.expand_as(M),))[1]

    tol = C_DERIV * D * torch.finfo(torch.float64).eps * (1 + float(M.abs().sum(-2).amax()))
    assert torch.allclose(e, torch.linalg.matrix_exp(M), rtol=tol, atol=tol * float(e.abs().max()))
    for f in range(F):
        t = L(B[f])
        assert float((dX[:, f] - t).abs().max()) <= tol * float(t.abs().max()) * 4
    for f, gg in ((0, 0), (1, 3), (4, 2)):
        t = jvp(lambda m: jvp(torch.linalg.matrix_exp, (m,), (B[f].expand_as(m),))[1], (M,), (B[gg].expand_as(M),))[1]
        assert float((hX[:, f, gg] - t).abs().max()) <= tol * float(t.abs().max()) * 4
    assert torch.equal(hX, hX.transpose(1, 2))
    one = torch.eye(D * D, dtype=torch.float64, device='cuda').reshape(D * D, D, D)
    Lij = torch.stack([L(one[k]) for k in range(D * D)], 1).reshape(3, 1, D, D, D, D)
    t = p.reshape(3, F, 1, 1, 1, 1) * Lij
    assert float((dB - t).abs().max()) <= tol * float(t.abs().max()) * 4


@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_gradcheck(N, D):
    gen = torch.Generator().manual_seed(D)
    x = (torch.randn(3, D, D, dtype=torch.float64, generator=gen) * 0.8).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda a: N.lie.expm(a), (x,))
    p = torch.randn(2, 4, dtype=torch.float64, generator=gen).cuda().requires_grad_()
    B = (torch.randn(4, D, D, dtype=torch.float64, generator=gen) * 0.5).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: N.lie.expm(a, b), (p, B))


def test_grad_matches_matrix_exp_float32(N):
    x = (torch.randn(1000, 3, 3) * 0.7).cuda().requires_grad_()
    g = torch.randn(1000, 3, 3).cuda()
    (gk,) = torch.autograd.grad(N.lie.expm(x), x, g)
    x64 = x.detach().double().requires_grad_()
    (gt,) = torch.autograd.grad(torch.linalg.matrix_exp(x64), x64, g.double())
    n1 = x64.detach().abs().sum(-2).amax(-1)
    err = (gk.double() - gt).abs().amax((-2, -1)) / gt.abs().amax((-2, -1))
    assert bool((err <= C_DERIV * 3 * torch.finfo(torch.float32).eps * (1 + n1) ** 2).all()), float(err.max())


@pytest.mark.parametrize('D', [9, 12, 16])
def test_large_orders_torch_route(N, D):
    x = (torch.randn(50, D, D, dtype=torch.float64) * 0.3).cuda()
    assert torch.equal(N.lie.expm(x), torch.linalg.matrix_exp(x))
    xg = x.clone().requires_grad_()
    N.lie.expm(xg).sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
    e, dX = N.lie.expm_derivatives(x[:2], grad_X=True)
    assert dX.shape == (2, D * D, D, D)


def test_empty_batch(N):
    x = torch.zeros(0, 4, 4, device='cuda')
    assert N.lie.expm(x).shape == (0, 4, 4)
    e, dX, hX = N.lie.expm_derivatives(x, grad_X=True, hess_X=True)
    assert dX.shape == (0, 16, 4, 4) and hX.shape == (0, 16, 16, 4, 4)
