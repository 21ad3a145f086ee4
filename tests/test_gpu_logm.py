"""`logm.logm` / `logm.meanm` on the MI355X: against the fixture's 40-digit truth and the reference's own outputs,
structure, scale, layouts, the NaN policy, streams, `logm(M^-1 A)`, autograd, the torch route and the barycentre.

Error of a result K against the truth T: max|K - T| / max|T|, per matrix.  The bound everywhere is
C_LOGM * D * eps * kappa_1(A), with C_LOGM from profiles/logm_accuracy.md."""
import os
import warnings
import numpy as np
import pytest
import torch
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# profiles/logm_accuracy.md: worst measured err / (D eps kappa_1) is 21.4 (float64 2x2 over 10^6 random matrices against
# the torch route, which carries an error of 11.6 of its own; 10.1 against mpmath on a sample), 18.2 against an exact
# truth (float32 3x3) and 18.6 for logm_solve; the next power of two at or above 4 x the worst.
C_LOGM = 128

DT = {'f32': torch.float32, 'f64': torch.float64}


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLDEN, 'logm.npz'))


@pytest.fixture(scope='module')
def LM():
    from nitorch_fastmath_amd import logm
    return logm


@pytest.fixture(scope='module')
def N():
    import nitorch_fastmath_amd as N
    return N


def rel(k, t):
    k, t = torch.as_tensor(k).double().cpu(), torch.as_tensor(t).double().cpu()
    return (k - t).abs().amax((-2, -1)) / t.abs().amax((-2, -1))


def bound(a, dtype, c=C_LOGM):
    a = torch.as_tensor(a).double().cpu()
    return c * a.shape[-1] * torch.finfo(dtype).eps * torch.linalg.cond(a, 1)


def spread(n, D, dtype, gen, scale=0.5):
    """A = expm(X), X = randn * scale"""
    x = torch.randn(n, D, D, dtype=torch.float64, generator=gen) * scale
    return torch.linalg.matrix_exp(x).to(dtype)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('D', range(1, 9))
def test_golden(LM, g, dt, D):
    x, ref, true = (torch.from_numpy(g[f'{k}_{dt}_{D}']) for k in ('x', 'ref', 'true'))
    dtype = DT[dt]
    k = LM.logm(x.cuda())
    assert k.dtype == dtype and k.is_contiguous()
    ek, er, b = rel(k, true), rel(ref, true), bound(x, dtype)
    print(dt, D, 'worst err / (D eps kappa)', float((ek / b).max()) * C_LOGM)
    assert bool((ek <= b).all()), float((ek / b).max())
    if dt == 'f64':
        assert bool((ek <= 2 * er + b).all())
    bad = torch.from_numpy(g[f'bad_{dt}_{D}'])
    assert torch.isnan(LM.logm(bad.cuda())).all()


def test_golden_bases(LM, g):
    for name in ('rigid', 'affine'):
        a, ref, true = (torch.from_numpy(g[f'{name}_{k}']) for k in ('x', 'ref', 'true'))
        k = LM.logm(a.cuda())
        b = bound(a, torch.float64)
        assert bool((rel(k, true) <= b).all()) and bool((rel(k, true) <= 2 * rel(ref, true) + b).all())
        assert float(k[:, 3].abs().max()) == 0          # the last row of the logarithm of a homogeneous matrix


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [2, 3, 4, 6, 8])
def test_structure(LM, N, dtype, D):
    gen = torch.Generator().manual_seed(D)
    I = torch.eye(D, dtype=torch.float64)
    a = spread(500, D, dtype, gen)
    la = LM.logm(a.cuda())
    b = bound(a, dtype)
    # expm(logm(A)) = A
    back = N.lie.expm(la.double()).cpu()
    assert bool((rel(back, a) <= b).all()), float((rel(back, a) / b).max())
    # logm(expm(X)) = X for ||X||_1 <= 1
    x = torch.randn(500, D, D, dtype=torch.float64, generator=gen)
    x = (x / x.abs().sum(-2).amax(-1)[:, None, None]).to(dtype)
    e = torch.linalg.matrix_exp(x.double())
    assert bool((rel(LM.logm(e.to(dtype).cuda()), x) <= bound(e, dtype)).all())
    # transpose, inverse
    assert bool((rel(LM.logm(a.mT.cuda()).mT, la) <= 2 * b).all())
    ai = torch.linalg.inv(a.double()).to(dtype)
    assert bool((rel(-LM.logm(ai.cuda()), la) <= 2 * b).all()), float((rel(-LM.logm(ai.cuda()), la) / b).max())
    # rotations: the logarithm is skew
    s = torch.randn(500, D, D, dtype=torch.float64, generator=gen)
    s = s - s.mT
    s = s * (2.5 / torch.linalg.eigvals(s).imag.abs().amax(-1))[:, None, None]
    r = torch.linalg.matrix_exp(s).to(dtype)
    lr = LM.logm(r.cuda()).double().cpu()
    assert bool(((lr + lr.mT).abs().amax((-2, -1)) <= bound(r, dtype) * lr.abs().amax((-2, -1))).all())
    # unipotent: the finite series log(I + N) = N - N^2/2 + ...
    n = torch.triu(torch.randn(500, D, D, dtype=torch.float64, generator=gen), 1).to(dtype).double()
    fs, p = torch.zeros_like(n), I.expand_as(n)
    for k in range(1, D):
        p = p @ n
        fs = fs + p * ((-1) ** (k + 1) / k)
    u = (I + n).to(dtype)
    assert bool((rel(LM.logm(u.cuda()), fs) <= bound(u, dtype)).all())
    z = LM.logm(torch.eye(D, dtype=dtype, device='cuda').expand(7, D, D))
    assert torch.equal(z.cpu(), torch.zeros(7, D, D, dtype=dtype))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_order_one_is_log(LM, dtype):
    x = torch.rand(1000, 1, 1, dtype=dtype).cuda() * 10 + 1e-3
    assert torch.allclose(LM.logm(x), torch.log(x), rtol=4 * torch.finfo(dtype).eps, atol=0)
    assert torch.isnan(LM.logm(-x)).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [3, 4])
def test_scale(LM, dtype, D):
    gen = torch.Generator(device='cuda').manual_seed(7)
    x = torch.randn(10 ** 6, D, D, dtype=torch.float64, device='cuda', generator=gen) * 0.5
    a = torch.linalg.matrix_exp(x).to(dtype)
    k = LM.logm(a).double()
    t = torch.cat([LM._logm_torch(c) for c in a.double().split(250000)])
    err = (k - t).abs().amax((-2, -1)) / t.abs().amax((-2, -1))
    kap = torch.linalg.cond(a.double(), 1)
    # float64: the torch route's own error is of the same order, hence twice the bound
    c = C_LOGM if dtype == torch.float32 else 2 * C_LOGM
    assert bool((err <= c * D * torch.finfo(dtype).eps * kap).all()), float((err / kap).max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [1, 3, 4, 7])
def test_layouts_bit_for_bit(LM, dtype, D):
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(301, D, D + 1, dtype=dtype, generator=gen) * 0.3
    base[..., :D] = torch.linalg.matrix_exp(base[..., :D].double()).to(dtype)
    base = base.cuda()
    f = LM.logm
    cases = [base[..., :D].mT, base[::2, :, :D], base[..., :D],                      # transposed, every other, padded
             base[:1, :, :D].expand(5, D, D), base[:, :, :D].reshape(7, 43, D, D),
             base[:1, :, :D], base[:0, :, :D]]
    for v in cases:
        out = f(v)
        assert out.is_contiguous() and out.shape == v.shape
        assert torch.equal(out, f(v.contiguous()))
        assert not torch.isnan(out).any()
    for n in (1, 63, 65, 257, 1001):
        x = spread(n, D, dtype, gen).cuda()
        assert torch.equal(f(x)[n // 2], f(x[n // 2:n // 2 + 1])[0])


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_policy(LM, dtype):
    gen = torch.Generator().manual_seed(5)
    x = spread(8, 3, dtype, gen)
    good = x.clone()
    x[1, 2, 1] = float('nan')
    x[2, 0, 0] = float('inf')
    x[3] = torch.diag(torch.tensor([0, 2, 3], dtype=dtype))
    x[4] = torch.diag(torch.tensor([-1, 2, 3], dtype=dtype))
    v = torch.tensor([[1.], [2.], [2.]], dtype=dtype) / 3
    x[5] = torch.eye(3, dtype=dtype) - 2 * v @ v.T                 # a reflection
    x[6] = torch.finfo(dtype).max / 8                               # huge, finite and singular: ends, NaN
    k = LM.logm(x.cuda()).cpu()
    assert torch.isnan(k[1:7]).all()
    # huge, finite and regular: 2^40 I takes its 25 or so steps per root; 2^80 I would need more than the 40 of Q22
    big = torch.eye(3, dtype=dtype) * torch.tensor([2.0 ** 40, 2.0 ** 80], dtype=dtype)[:, None, None]
    kb = LM.logm(big.cuda()).cpu()
    want = torch.eye(3, dtype=torch.float64) * 40 * np.log(2.0)
    assert float((kb[0].double() - want).abs().max()) <= C_LOGM * 3 * torch.finfo(dtype).eps * 40 * np.log(2.0)
    assert torch.isnan(kb[1]).all()
    assert torch.isfinite(k[0]).all() and torch.isfinite(k[7]).all()
    clean = LM.logm(good[[0, 7]].cuda()).cpu()
    assert torch.equal(k[[0, 7]], clean)
    for D in (2, 4):
        xx = torch.full((3, D, D), float('nan'), dtype=dtype).cuda()
        assert torch.isnan(LM.logm(xx)).all()
        assert torch.isnan(LM._frechet(xx, xx)).all()
    # the torch route has the same policy
    t = LM._logm_torch(x[:6].cuda()).cpu()
    assert torch.isnan(t[1:6]).all() and torch.isfinite(t[0]).all()


def test_side_stream(LM):
    x = torch.linalg.matrix_exp(torch.randn(5000, 4, 4, device='cuda') * 0.5)
    ref = LM.logm(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = LM.logm(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_empty_batch(LM):
    x = torch.zeros(0, 4, 4, device='cuda')
    assert LM.logm(x).shape == (0, 4, 4)
    assert LM._logm(x, x).shape == (0, 4, 4)
    assert LM.logm(torch.zeros(3, 0, 12, 12, device='cuda')).shape == (3, 0, 12, 12)


@pytest.mark.parametrize('D', [9, 12, 16])
def test_large_orders_torch_route(LM, D):
    gen = torch.Generator().manual_seed(D)
    a = spread(50, D, torch.float64, gen, 0.3).cuda()
    k = LM.logm(a)
    back = torch.linalg.matrix_exp(k)
    assert bool((rel(back, a) <= 2 * bound(a, torch.float64) * k.cpu().abs().amax((-2, -1)).clamp_min(1)).all())
    k32 = LM.logm(a.float())
    assert k32.dtype == torch.float32 and bool((rel(k32, k) <= bound(a, torch.float32)).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [2, 3, 4, 7])
def test_logm_solve(LM, dtype, D):
    gen = torch.Generator().manual_seed(D)
    # (small enough that M^-1 A keeps its eigenvalues off the negative real axis)
    a = spread(300, D, dtype, gen, 0.9 / D).cuda()
    for m in (spread(1, D, dtype, gen, 0.6 / D).cuda(), spread(300, D, dtype, gen, 0.6 / D).cuda()):
        k = LM._logm(a, m)
        q = torch.linalg.solve(m.double(), a.double())
        t = LM._logm_torch(q)
        b = bound(q, dtype)
        print(dtype, D, 'logm_solve worst err / (D eps kappa)', float((rel(k, t) / b).max()) * C_LOGM)
        assert bool((rel(k, t) <= b).all()), float((rel(k, t) / b).max())
    assert torch.equal(LM._logm(a, m[:1]), LM._logm(a, m[:1].expand_as(a).contiguous()))


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_gradcheck(LM, D):
    gen = torch.Generator().manual_seed(D)
    x = spread(3, D, torch.float64, gen).cuda().requires_grad_()
    assert torch.autograd.gradcheck(LM.logm, (x,))


def test_grad_float32_against_float64(LM):
    gen = torch.Generator().manual_seed(1)
    x = spread(1000, 3, torch.float32, gen).cuda().requires_grad_()
    gg = torch.randn(1000, 3, 3, generator=gen).cuda()
    (gk,) = torch.autograd.grad(LM.logm(x), x, gg)
    x64 = x.detach().double().requires_grad_()
    (gt,) = torch.autograd.grad(LM.logm(x64), x64, gg.double())
    err = (gk.double() - gt).abs().amax((-2, -1)) / gt.abs().amax((-2, -1))
    kap = torch.linalg.cond(x64.detach(), 1)
    # the derivative of the logarithm involves the inverse once more than the logarithm: kappa^2
    assert bool((err <= C_LOGM * 3 * torch.finfo(torch.float32).eps * kap ** 2).all()), float((err / kap ** 2).max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('D', [2, 3, 4, 5])
def test_frechet_against_jvp(LM, dtype, D):
    from torch.func import jvp
    gen = torch.Generator().manual_seed(D)
    x = spread(200, D, dtype, gen).cuda()
    d = torch.randn(200, D, D, dtype=torch.float64, generator=gen).to(dtype).cuda()
    k = LM._frechet(x, d)
    t = jvp(LM._logm_torch, (x.double(),), (d.double(),))[1]
    kap = torch.linalg.cond(x.double(), 1).cpu()
    err = rel(k, t)
    assert bool((err <= C_LOGM * D * torch.finfo(dtype).eps * kap ** 2).all()), float((err / kap ** 2).max())
    # the adjoint is the same call at the transpose: <L(X^T, G), H> = <G, L(X, H)>, per matrix
    h = torch.randn(200, D, D, dtype=torch.float64, generator=gen).to(dtype).cuda()
    lhs = (LM._frechet(x.mT, d).double() * h.double()).sum((-2, -1)).cpu()
    rhs = (d.double() * LM._frechet(x, h).double()).sum((-2, -1)).cpu()
    scale = (d.double().norm(dim=(-2, -1)) * LM._frechet(x, h).double().norm(dim=(-2, -1))).cpu()
    assert bool(((lhs - rhs).abs() <= C_LOGM * D * torch.finfo(dtype).eps * kap ** 2 * scale).all())


def _sos(LM, mean, mats):
    logs = LM._logm_torch(torch.linalg.solve(mean.double(), mats.double()))
    return logs.mean(-3).square().sum((-2, -1))


def test_meanm_golden(LM, g):
    tol = 1e-20
    for name in ('rigid', 'affine', 'spd'):
        mats, ref, sos_ref = (torch.from_numpy(g[f'meanm_{name}_{k}']) for k in ('x', 'ref', 'sos'))
        k = LM.meanm(mats.cuda())
        assert k.shape == ref.shape and k.dtype == torch.float64
        kap = torch.linalg.cond(mats, 1).max()
        assert float(rel(k, ref)) <= C_LOGM * mats.shape[-1] * torch.finfo(torch.float64).eps * float(kap)
        sos = float(_sos(LM, k, mats.cuda()))
        print(name, 'sos', sos, 'reference', float(sos_ref))
        assert sos <= max(tol, 10 * float(sos_ref))


def test_meanm_properties(LM, N):
    gen = torch.Generator().manual_seed(2)
    a = spread(1, 4, torch.float64, gen)[0]
    pair = torch.stack([a, torch.linalg.inv(a)]).cuda()
    m = LM.meanm(pair).cpu()
    assert float((m - torch.eye(4, dtype=torch.float64)).abs().max()) <= 1e-12
    x = torch.randn(3, 3, dtype=torch.float64, generator=gen) * 0.3
    w = torch.rand(9, dtype=torch.float64, generator=gen)
    mats = torch.linalg.matrix_exp(w[:, None, None] * x)
    m = LM.meanm(mats.cuda()).cpu()
    assert float((m - torch.linalg.matrix_exp(w.mean() * x)).abs().max()) <= 1e-12
    # a list, and float32 in -> float32 out
    ml = LM.meanm([t.cuda() for t in mats])
    assert torch.equal(ml.cpu(), m)
    m32 = LM.meanm(mats.float().cuda())
    assert m32.dtype == torch.float32 and float((m32.double().cpu() - m).abs().max()) <= 1e-5


def test_meanm_batched_equals_the_loop(LM):
    gen = torch.Generator().manual_seed(4)
    sets = spread(5 * 16, 4, torch.float64, gen, 0.4).reshape(5, 16, 4, 4)
    sets[2] = torch.eye(4, dtype=torch.float64)              # converges at once: stops updating first
    sets = sets.cuda()
    both = LM.meanm(sets)
    assert both.shape == (5, 4, 4)
    for q in range(5):
        assert torch.equal(both[q], LM.meanm(sets[q])), q


def test_meanm_warns_on_a_matrix_without_a_real_logarithm(LM):
    gen = torch.Generator().manual_seed(6)
    mats = spread(6, 3, torch.float64, gen)
    mats[3] = torch.diag(torch.tensor([-1., 2., 3.], dtype=torch.float64))
    with pytest.warns(RuntimeWarning, match='failed to converge'):
        m = LM.meanm(mats.cuda())
    assert m.shape == (3, 3)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        LM.meanm(mats[:3].cuda())
