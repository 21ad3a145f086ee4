"""`logm`, `logm_solve`, the Frechet kernel and `LogmFn`'s backward on hard inputs, per record, against the validated
truths of tests/golden/logm_hard.npz (classes, tiers and bounds: tests/_logm_ref.py).

The batches interleave every class of both tiers with an identity and four records without a real logarithm and
cycle them to 1, 63, 64, 65 and 257 matrices: neighbouring lanes then need 0, a few and dozens of Denman-Beavers
steps and restart their square roots at different passes of the flattened loop, over one wave and over several.
"""
import numpy as np
import pytest
import torch
import _logm_ref as R

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
LENGTHS = (1, 63, 64, 65, 257)
CASES = [(dt, D) for dt in R.ORDERS for D in R.ORDERS[dt]]
FRECHET_CASES = [(dt, D) for dt in R.ORDERS for D in R.FRECHET_ORDERS]
N_BAD = 4


@pytest.fixture(scope='module')
def g():
    return R.load()


@pytest.fixture(scope='module')
def LM():
    from nitorch_fastmath_amd import logm
    return logm


def specials(D, dtype):
    """identity, then N_BAD records without a real logarithm: a NaN entry, singular, diag(-1, 2, ..), an inf entry"""
    eye = torch.eye(D, dtype=dtype)
    d = torch.arange(1, D + 1, dtype=dtype)
    nan = eye.clone()
    nan[-1, 0] = float('nan')
    sing = torch.diag(d.clone())
    sing[0, 0] = 0
    neg = torch.diag(d.clone())
    neg[0, 0] = -1
    inf = eye.clone()
    inf[0, -1] = float('inf')
    return torch.stack([eye, nan, sing, neg, inf])


def base(rec, dtype):
    """the fixture's records with their classes interleaved, then the specials -> (matrices, order of the records)"""
    x = torch.from_numpy(rec['x'])
    n = len(x)
    # the fixture is class by class, PER_CLASS records each: take one of every class in turn
    order = np.arange(n).reshape(-1, R.PER_CLASS).T.ravel()
    return torch.cat([x[order], specials(x.shape[-1], dtype)]), order


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def alone(f, *ops):
    """every record computed in a launch of its own"""
    return torch.cat([f(*[o[i:i + 1] for o in ops]) for i in range(len(ops[0]))])


def check_specials(out, nrec):
    assert torch.equal(out[nrec].cpu(), torch.zeros_like(out[nrec]).cpu())
    assert torch.isnan(out[nrec + 1:nrec + 1 + N_BAD]).all()


@pytest.mark.parametrize('dt,D', CASES)
def test_logm_mixed_batches(LM, g, dt, D):
    """tier A within C_LOGM eps m, tier B NaN or within C_LOGM eps m^2, every lane of every batch equal to the
    record computed alone; the records without a logarithm are NaN and leave their neighbours unchanged"""
    rec = R.records(g, dt, D)
    b, order = base(rec, DT[dt])
    b = b.cuda()
    nrec = len(order)
    one = alone(LM.logm, b)
    check_specials(one, nrec)
    ok, r, what = R.check_logm(one[:nrec].cpu().numpy(), {k: v[order] for k, v in rec.items()}, dt)
    sub = {k: v[order] for k, v in rec.items()}
    print(dt, D, 'logm worst err / (eps m):', {k: f'{v:.3g}' for k, v in R.worst_by_class(r, sub).items()})
    print(dt, D, 'tier B:', [(sub['cls'][i], float(sub['par'][i]), what[i], f'{r[i] / R.m_of(sub["cl"][i]):.3g}')
                             for i in range(nrec) if sub['tier'][i] == R.TIER_B])
    assert ok.all(), [(sub['cls'][i], float(sub['par'][i]), what[i], float(r[i])) for i in np.flatnonzero(~ok)]
    for n in LENGTHS:
        idx = torch.arange(n) % len(b)
        out = LM.logm(b[idx.cuda()])
        assert same_bits(out, one[idx.cuda()]), n


@pytest.mark.parametrize('dt,D', CASES)
def test_logm_solve(LM, g, dt, D):
    """log(M^-1 A), M graded and A of every tier-A class, within C_LOGM D eps kappa_1(M) max(1, cond_log(M^-1 A));
    M per record and M at stride 0, over two waves, every lane equal to the pair computed alone"""
    sm, sa, true, kap, cl = (g[f'{k}_{dt}_{D}'] for k in ('sm', 'sa', 'strue', 'skap', 'scl'))
    m, a = torch.from_numpy(sm).cuda(), torch.from_numpy(sa).cuda()
    one = alone(LM._logm, a, m)
    k = one.double().cpu().numpy()
    assert np.isfinite(k).all()
    r = R.fro(k - true) / R.fro(true) / (D * R.EPS[dt] * kap * R.m_of(cl))
    print(dt, D, 'logm_solve err / (D eps kappa_1(M) m):', dict(zip(g[f'scls_{dt}_{D}'].tolist(), np.round(r, 3))))
    assert (r <= R.C_LOGM).all(), r
    idx = (torch.arange(65) % len(a)).cuda()
    assert same_bits(LM._logm(a[idx], m[idx]), one[idx])
    for j in range(len(a)):
        # one M for the whole batch, read at stride 0
        out = LM._logm(a[j:j + 1].expand(65, D, D).contiguous(), m[j:j + 1])
        assert same_bits(out, one[j:j + 1].expand(65, D, D))
    # the mixed batch of `logm` under one M each: whatever M^-1 A is, a lane does not depend on its neighbours
    b = base(R.records(g, dt, D), DT[dt])[0].cuda()
    mm = m[(torch.arange(len(b)) % len(m)).cuda()]
    ref = alone(LM._logm, b, mm)
    assert torch.isnan(ref[-N_BAD:]).all()
    for n in LENGTHS:
        idx = (torch.arange(n) % len(b)).cuda()
        assert same_bits(LM._logm(b[idx], mm[idx]), ref[idx]), n


@pytest.mark.parametrize('dt,D', FRECHET_CASES)
def test_frechet_mixed_batches(LM, g, dt, D):
    """tier A within C_LOGM D eps m^2 ||K||_2 ||E||_F of the validated derivative; tier B NaN or finite (printed);
    every lane of every batch equal to the record computed alone"""
    rec = R.records(g, dt, D)
    b, order = base(rec, DT[dt])
    nrec = len(order)
    sub = {k: v[order] for k, v in rec.items()}
    gen = torch.Generator().manual_seed(D)
    e = torch.cat([torch.from_numpy(sub['E']), torch.randn(1 + N_BAD, D, D, generator=gen, dtype=DT[dt])])
    b, e = b.cuda(), e.cuda()
    one = alone(LM._frechet, b, e)
    assert torch.isnan(one[nrec + 1:]).all() and torch.isfinite(one[nrec]).all()
    l = one[:nrec].double().cpu().numpy()
    r = R.frechet_ratio(l, sub, dt)
    ta = sub['tier'] == R.TIER_A
    print(dt, D, 'frechet worst err / (D eps m^2 ||K|| ||E||):',
          {k: f'{v:.3g}' for k, v in R.worst_by_class(r, sub).items()})
    print(dt, D, 'tier B:', [(sub['cls'][i], float(sub['par'][i]),
                              'nan' if np.isnan(l[i]).all() else 'finite' if np.isfinite(l[i]).all() else 'mixed')
                             for i in np.flatnonzero(~ta)])
    assert np.isfinite(l[ta]).all()
    assert (r[ta] <= R.C_LOGM).all(), [(sub['cls'][i], float(sub['par'][i]), float(r[i]))
                                       for i in np.flatnonzero(ta & ~(r <= R.C_LOGM))]
    for i in np.flatnonzero(~ta):
        assert np.isnan(l[i]).all() or np.isfinite(l[i]).all()
    for n in LENGTHS:
        idx = (torch.arange(n) % len(b)).cuda()
        assert same_bits(LM._frechet(b[idx], e[idx]), one[idx]), n


@pytest.mark.parametrize('dt,D', FRECHET_CASES)
def test_backward_is_the_adjoint_of_the_true_derivative(LM, g, dt, D):
    """<backward(X, G), E> = <G, L_log(X, E)> on tier A, within C_LOGM D eps m^2 ||K||_2 ||E||_F ||G||_F"""
    rec = R.records(g, dt, D)
    ta = rec['tier'] == R.TIER_A
    sub = {k: v[ta] for k, v in rec.items()}
    x = torch.from_numpy(sub['x']).cuda().requires_grad_()
    gen = torch.Generator().manual_seed(10 + D)
    G = torch.randn(x.shape, generator=gen, dtype=torch.float64).to(DT[dt])
    (gx,) = torch.autograd.grad(LM.logm(x), x, G.cuda())
    gx, G = gx.double().cpu().numpy(), G.double().numpy()
    lhs = (gx * sub['E'].astype(np.float64)).sum((-2, -1))
    rhs = (G * sub['L']).sum((-2, -1))
    r = np.abs(lhs - rhs) / (D * R.EPS[dt] * R.m_of(sub['cl']) ** 2 * sub['nK'] * R.fro(sub['E']) * R.fro(G))
    print(dt, D, 'backward worst |<gx, E> - <G, L>| / (D eps m^2 ||K|| ||E|| ||G||):',
          {k: f'{v:.3g}' for k, v in R.worst_by_class(r, sub).items()})
    assert np.isfinite(gx).all() and (r <= R.C_LOGM).all(), r


@pytest.mark.parametrize('dt,D', [(dt, D) for dt in R.ROUTE_ORDERS for D in R.ROUTE_ORDERS[dt]])
def test_torch_route(LM, g, dt, D):
    """the orders without a kernel on the tier-A constructions: float64 against the truth, float32 against the
    float64 route on the same input (and the truth)"""
    rec = R.records(g, dt, D)
    assert (rec['tier'] == R.TIER_A).all()
    x = torch.from_numpy(rec['x']).cuda()
    k = LM.logm(x)
    assert k.dtype == DT[dt]
    ok, r, what = R.check_logm(k.cpu().numpy(), rec, dt)
    print(dt, D, 'route worst err / (eps m):', {c: f'{v:.3g}' for c, v in R.worst_by_class(r, rec).items()})
    assert ok.all(), list(zip(rec['cls'], r))
    if dt == 'f32':
        k64 = LM.logm(x.double())
        r = R.fro((k.double() - k64).cpu().numpy()) / R.fro(k64.cpu().numpy()) / (R.EPS[dt] * R.m_of(rec['cl']))
        assert torch.isfinite(k64).all() and (r <= R.C_LOGM).all(), r
