"""GPU checks of the stochastic module: the probe streams against the numpy model (bit for bit for +-1), gram and
combine against float64 numpy with bounds from the arithmetic they promise, the Gram-Schmidt orthogonalisation
against Householder QR, and the three public functions (tests/_stochastic_ref.py holds the model).

Every bound is a statement about arithmetic, none is fitted:
  gram     sums of exact-or-once-rounded products in double, any order:  |err| <= n eps64 sum |x_i y_i|
  combine  p fused multiply-adds in double + one rounding to the dtype:  (p + 2) eps (|y| + sum |x| |c|)
  fill     1-ulp log, 1/2-ulp sqrt, 2-ulp sincospi, one product:         8 eps max(1, r)
Worst observed fractions of these bounds: profiles/stochastic_accuracy.md."""
import functools
import json
import math
import os
import numpy as np
import pytest
import torch
from conftest import GOLDEN
import _stochastic_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 129, 1027, 2 ** 16 + 3]
BIG = 2 ** 23 + 5                       # past one pass of the fixed grid (2048 workgroups x 256 lanes x 16 bytes)
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
SEED = 0x1234567887654321 & (2 ** 62 - 1)


def S():
    import nitorch_fastmath_amd as N
    return N.stochastic


def L():
    from nitorch_fastmath_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def model_rademacher(offset, n):
    return R.rademacher(SEED, offset, n)


@functools.lru_cache(maxsize=None)
def model_gaussian(offset, n):
    return R.gaussian(SEED, offset, n, return_radius=True)


def f64(t):
    return t.detach().cpu().double().numpy()


# ------------------------------------------------------------------------------------------- fill
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('offset', [0, 2 ** 40 + 77])
def test_fill_rademacher_is_the_model_bit_for_bit(dev, dn, offset):
    for n in SIZES + ([BIG] if dn == 'f32' else []):
        want = model_rademacher(offset, n)
        buf = torch.zeros(n + 9, dtype=DT[dn], device=dev)
        S()._fill(buf[:n], L().STOCH_RADEMACHER, SEED, offset)                       # aligned base
        assert np.array_equal(f64(buf[:n]), want), (n, 'aligned')
        assert float(buf[n:].abs().max()) == 0.0, (n, 'wrote past the end')
        buf.zero_()
        S()._fill(buf[1:n + 1], L().STOCH_RADEMACHER, SEED, offset)                  # odd element offset
        assert np.array_equal(f64(buf[1:n + 1]), want), (n, 'odd base')
        assert float(buf[0]) == 0.0 and float(buf[n + 1:].abs().max()) == 0.0, (n, 'wrote outside')
        buf.zero_()
        k = (n * 5) // 13                                                            # the range in two calls
        if k:
            S()._fill(buf[:k], L().STOCH_RADEMACHER, SEED, offset)
        S()._fill(buf[k:n], L().STOCH_RADEMACHER, SEED, offset + k)
        assert np.array_equal(f64(buf[:n]), want), (n, 'split at', k)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('offset', [0, 2 ** 40 + 77])
def test_fill_gaussian_is_the_model_to_rounding(dev, dn, offset):
    worst = 0.0
    for n in SIZES + ([BIG] if (dn == 'f32' and offset == 0) else []):
        want, rad = model_gaussian(offset, n)
        bound = 8 * EPS[dn] * np.maximum(1.0, rad)
        buf = torch.zeros(n + 9, dtype=DT[dn], device=dev)
        S()._fill(buf[:n], L().STOCH_GAUSSIAN, SEED, offset)
        a = f64(buf[:n])
        S()._fill(buf[1:n + 1], L().STOCH_GAUSSIAN, SEED, offset)                    # odd base: the same bits
        assert np.array_equal(f64(buf[1:n + 1]), a), n
        assert float(buf[n + 1:].abs().max()) == 0.0, n
        k = (n * 5) // 13
        if k:
            S()._fill(buf[:k], L().STOCH_GAUSSIAN, SEED, offset)
        S()._fill(buf[k:n], L().STOCH_GAUSSIAN, SEED, offset + k)
        assert np.array_equal(f64(buf[:n]), a), (n, 'split at', k)
        ratio = float((np.abs(a - want) / bound).max())
        worst = max(worst, ratio)
        print(f'gaussian {dn} offset {offset} n {n}: worst |err| / bound = {ratio:.3f}')
        assert ratio <= 1.0, (n, ratio)
    print(f'gaussian {dn} offset {offset}: worst ratio {worst:.3f}')


@pytest.mark.parametrize('kind', ['rademacher', 'gaussian'])
def test_a_stack_of_samples_is_the_single_fills(dev, kind):
    k, n = L().STOCH_RADEMACHER if kind[0] == 'r' else L().STOCH_GAUSSIAN, 1027
    stack = S()._fill(torch.empty(3, n, device=dev), k, SEED)
    for i in range(3):
        assert torch.equal(stack[i], S()._fill(torch.empty(n, device=dev), k, SEED, i * n))
    model = R.probes(kind, SEED, 3, n)
    if kind[0] == 'r':
        assert np.array_equal(f64(stack), model)
    else:
        assert np.abs(f64(stack) - model).max() <= 8 * EPS['f32'] * 6


# ------------------------------------------------------------------------------------------- gram
def exact_gram(x, y):
    """sum_i x_j[i] y_k[i] in extended precision (pairwise, 64-bit mantissa), and sum_i |x_j[i] y_k[i]|"""
    xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
    g = np.array([[np.sum(a * b) for b in yl] for a in xl])
    s = np.array([[np.sum(np.abs(a * b)) for b in yl] for a in xl])
    return g, s


def vectors(rng, count, n, dn):
    return (rng.standard_normal((count, n)) * np.exp(rng.uniform(-3, 3, (count, 1)))).astype(NP[dn])


def run_gram(xs, ys, dev, out=None, accumulate=False):
    xt = [torch.as_tensor(v, device=dev) if not torch.is_tensor(v) else v for v in xs]
    yt = [torch.as_tensor(v, device=dev) if not torch.is_tensor(v) else v for v in ys]
    if out is None:
        out = torch.full((len(xt) * len(yt),), float('nan'), dtype=torch.float64, device=dev)
    return S()._gram(xt, yt, out, accumulate)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('p,q', [(1, 1), (2, 1), (8, 1), (4, 4), (8, 8), (3, 5), (1, 3)])
def test_gram_against_exact_sums(dev, dn, p, q):
    rng = np.random.default_rng(p * 16 + q)
    for n in SIZES + ([BIG] if (dn == 'f32' and (p, q) in [(1, 1), (4, 4)]) else []):
        x, y = vectors(rng, p, n, dn), vectors(rng, q, n, dn)
        got = run_gram(list(x), list(y), dev).cpu().numpy().reshape(p, q)
        want, mass = exact_gram(x, y)
        err = np.abs(got - want.astype(np.float64))
        bound = n * EPS['f64'] * mass.astype(np.float64)
        print(f'gram {dn} ({p},{q}) n {n}: worst err / bound = {float((err / bound).max()):.2e}')
        assert (err <= bound).all(), (n, (err / bound).max())


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_gram_sums_in_double_on_a_cancelling_input(dev, dn):
    """x = +-1, y = +- x (1 + 1e-3 g) with alternating sign: the sum is ~1e-3 sqrt(n) while sum |x y| = n;
    accumulating in float32 would miss the bound by orders of magnitude"""
    n = 2 ** 16 + 3
    x = R.rademacher(SEED, 0, n)
    y = x * (1 + 1e-3 * R.gaussian(SEED, 0, n)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    x, y = x.astype(NP[dn]), y.astype(NP[dn])
    got = float(run_gram([x], [y], dev))
    want, mass = exact_gram(x[None], y[None])
    bound = n * EPS['f64'] * float(mass[0, 0])
    assert abs(got - float(want[0, 0])) <= bound
    if dn == 'f32':
        naive = float(torch.as_tensor(x).dot(torch.as_tensor(y)))          # float32 accumulation, for the record
        print(f'cancelling input: |err| {abs(got - float(want[0, 0])):.2e}, bound {bound:.2e}, '
              f'a float32 dot is off by {abs(naive - float(want[0, 0])):.2e}')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_gram_accumulates_repeats_and_ignores_alignment(dev, dn):
    rng = np.random.default_rng(5)
    for (p, q), n in [((1, 1), 63), ((2, 1), 1027), ((4, 4), 1027), ((3, 5), 129), ((8, 8), 2 ** 16 + 3)]:
        # rows of an odd-length stack: every row but the first sits off the 16-byte grid
        stack = torch.as_tensor(vectors(rng, p + q, n, dn), device=dev)
        xs, ys = [stack[j] for j in range(p)], [stack[p + k] for k in range(q)]
        assert any(t.data_ptr() % 16 for t in xs + ys)
        a = run_gram(xs, ys, dev)
        assert torch.equal(a, run_gram(xs, ys, dev))                               # two calls, the same bits
        b = run_gram([t.clone() for t in xs], [t.clone() for t in ys], dev)        # separately allocated copies
        assert all(t.data_ptr() % 16 == 0 for t in [xs[0].clone()])
        assert torch.equal(a, b), ((p, q), n)
        base = torch.arange(1, p * q + 1, dtype=torch.float64, device=dev) * 1.5
        acc = run_gram(xs, ys, dev, out=base.clone(), accumulate=True)
        assert torch.equal(acc, base + a)
        # a view into a larger float64 array is a valid output
        hist = torch.zeros(4, p * q, dtype=torch.float64, device=dev)
        run_gram(xs, ys, dev, out=hist[2])
        assert torch.equal(hist[2], a) and float(hist[[0, 1, 3]].abs().max()) == 0.0


def test_gram_of_nothing_is_zero(dev):
    e = torch.empty(0, device=dev)
    out = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    assert float(S()._gram([e], [e], out)) == 0.0
    out.fill_(7.0)
    assert float(S()._gram([e], [e], out, accumulate=True)) == 7.0


# ---------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('p,q', [(0, 1), (1, 1), (3, 1), (8, 1), (2, 2), (4, 4), (8, 8), (3, 5), (0, 3)])
def test_combine_elementwise(dev, dn, p, q):
    rng = np.random.default_rng(100 + p * 16 + q)
    for n in [1, 63, 129, 1027, 2 ** 16 + 3] + ([BIG] if (dn == 'f32' and (p, q) == (1, 1)) else []):
        x, y = vectors(rng, p, n, dn), vectors(rng, q, n, dn)
        c = rng.standard_normal((p, q))
        xt, yt = torch.as_tensor(x, device=dev), torch.as_tensor(y, device=dev)
        ct = torch.as_tensor(c, device=dev).reshape(-1)
        zt = torch.full((q, n + 3), 9.0, dtype=DT[dn], device=dev)          # rows off the 16-byte grid, with a guard
        zs = [zt[k, 1:n + 1] for k in range(q)]
        S()._combine([xt[j] for j in range(p)], ct if p else None, [yt[k] for k in range(q)], zs)
        want = y.astype(np.float64) - np.einsum('jn,jk->kn', x.astype(np.float64), c)
        bound = (p + 2) * EPS[dn] * (np.abs(y) + np.einsum('jn,jk->kn', np.abs(x).astype(np.float64), np.abs(c)))
        got = f64(zt[:, 1:n + 1])
        print(f'combine {dn} ({p},{q}) n {n}: worst err / bound = {float((np.abs(got - want) / bound).max()):.3f}')
        assert (np.abs(got - want) <= bound).all(), (n, (np.abs(got - want) / bound).max())
        assert float((zt[:, 0] - 9).abs().max()) == 0.0 and float((zt[:, n + 1:] - 9).abs().max()) == 0.0
        # in place: Z aliasing Y gives the same bits
        ys = [yt[k] for k in range(q)]
        S()._combine([xt[j] for j in range(p)], ct if p else None, ys, ys)
        assert torch.equal(yt, zt[:, 1:n + 1]), n


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_combine_scales_from_device_memory(dev, dn):
    n, eps = 1027, EPS[dn]
    y = torch.as_tensor(vectors(np.random.default_rng(3), 1, n, dn)[0], device=dev)
    s = torch.tensor([3.7], dtype=torch.float64, device=dev)
    z = torch.empty_like(y)
    S()._combine([], None, [y], [z], L().STOCH_SCALE_RSQRT, None, s)
    # sqrt, reciprocal and product in double + the store here, two roundings in `want`: under 3 eps
    want = f64(y) / math.sqrt(3.7)
    assert (np.abs(f64(z) - want) <= 3 * eps * np.abs(want)).all()
    thr = (64 * eps) ** 2
    ref = torch.tensor([5.0], dtype=torch.float64, device=dev)
    for sv, keep in [(5.0 * thr * 1.01, True), (5.0 * thr * 0.99, False), (0.0, False), (-1.0, False),
                     (float('nan'), False), (float('inf'), False), (2.0, True)]:
        s.fill_(sv)
        z.fill_(9.0)
        S()._combine([], None, [y], [z], L().STOCH_SCALE_RSQRT_OR_DROP, ref, s)
        if keep:
            want = f64(y) / math.sqrt(sv)
            assert (np.abs(f64(z) - want) <= 3 * eps * np.abs(want)).all(), sv
        else:
            assert float(z.abs().max()) == 0.0, sv
    # with a projection in the same launch
    x = torch.as_tensor(vectors(np.random.default_rng(4), 2, n, dn), device=dev)
    c = torch.tensor([0.5, -2.0], dtype=torch.float64, device=dev)
    s.fill_(4.0)
    S()._combine([x[0], x[1]], c, [y], [z], L().STOCH_SCALE_RSQRT, None, s)
    want = (f64(y) - 0.5 * f64(x[0]) + 2.0 * f64(x[1])) / 2
    bound = 5 * eps * (np.abs(f64(y)) + 0.5 * np.abs(f64(x[0])) + 2 * np.abs(f64(x[1]))) / 2
    assert (np.abs(f64(z) - want) <= bound).all()


# ------------------------------------------------------------------------------------------- orth
def conditioned(rng, n, m, cond):
    u = np.linalg.qr(rng.standard_normal((n, m)))[0]
    v = np.linalg.qr(rng.standard_normal((m, m)))[0]
    return (u * np.logspace(0, -math.log10(cond), m)) @ v.T                 # (n, m)


def loss(q):
    q = np.asarray(q, dtype=np.float64)
    return float(np.abs(q.T @ q - np.eye(q.shape[1])).max()) if q.shape[1] else 0.0


@pytest.mark.parametrize('m', [2, 4, 8])
@pytest.mark.parametrize('dn,cond,may_drop', [('f32', 1e3, False), ('f64', 1e7, False), ('f32', 1e6, True), ('f64', 1e12, True)])
def test_orth_against_householder(dev, dn, cond, may_drop, m):
    n = 1027
    y = conditioned(np.random.default_rng(m), n, m, cond).astype(NP[dn])
    q = torch.as_tensor(y.T.copy(), device=dev)                              # (m, n): rows are the columns
    norms = S()._orth(q)
    q = f64(q).T
    kept = [j for j in range(m) if np.any(q[:, j] != 0)]
    if not may_drop:
        assert kept == list(range(m))
    assert 0 in kept and len(kept) >= 1
    loss_ref = loss(np.linalg.qr(y.astype(np.float64))[0].astype(NP[dn]))
    got = loss(q[:, kept])
    print(f'orth {dn} cond {cond:g} m {m}: kept {len(kept)}, loss {got:.2e}, householder {loss_ref:.2e}, '
          f'fraction of bound {got / (2 * loss_ref + 4 * m * EPS[dn]):.2e}')
    assert got <= 2 * loss_ref + 4 * m * EPS[dn]
    # a projection never lengthens a column
    nn = norms.cpu().numpy()
    assert (nn[:, 1] <= nn[:, 0] * (1 + 1e-6)).all()


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_orth_zeroes_dependent_columns_exactly(dev, dn):
    rng = np.random.default_rng(9)
    n = 1027
    y = rng.standard_normal((3, n)).astype(NP[dn])
    y[2] = y[0] + y[1]
    q = torch.as_tensor(y, device=dev)
    S()._orth(q)
    assert float(q[2].abs().max()) == 0.0 and float(q[0].abs().max()) > 0 and float(q[1].abs().max()) > 0
    y = rng.standard_normal((8, n)).astype(NP[dn])
    y[3] = 2 * y[0] - 0.5 * y[1]
    y[6] = y[2] + 3 * y[4] - y[5]
    q = torch.as_tensor(y, device=dev)
    S()._orth(q)
    dropped = [j for j in range(8) if float(q[j].abs().max()) == 0.0]
    assert dropped == [3, 6]
    kept = f64(q)[[0, 1, 2, 4, 5, 7]].T
    assert loss(kept) <= 4 * 8 * EPS[dn] + 2 * loss(np.linalg.qr(y[[0, 1, 2, 4, 5, 7]].T.astype(np.float64))[0].astype(NP[dn]))


# --------------------------------------------------------------------------------------- trapprox
def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(seed):
    """the 62-bit probe seed a public call draws from gen(seed)"""
    return int(torch.randint(0, 2 ** 62, (1,), generator=gen(seed)))


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_trapprox_rademacher_on_a_diagonal_operator_is_exact(dev, dn):
    """v^2 = 1: every moment comes out exactly, up to j roundings of lambda^j v in the dtype and the double sum"""
    n = 2 ** 16 + 3
    lam = torch.linspace(0.2, 1.5, n, dtype=DT[dn])
    lam_d = lam.to(dev)
    t = S().trapprox(lambda x: x * lam_d, [n], moments=5, samples=3, dtype=DT[dn], device=dev)
    assert t.dtype == DT[dn] and t.shape == (5,) and t.device.type == 'cuda'
    t64 = S()._moments(lambda x: x * lam_d, [n], 5, 3, L().STOCH_RADEMACHER, False, DT[dn], dev, SEED).cpu().numpy()
    l64 = lam.double().numpy()
    for j in range(1, 6):
        truth = float(np.sum(l64 ** j))
        assert abs(t64[j - 1] - truth) <= (j * EPS[dn] + n * EPS['f64']) * truth, j
        assert abs(float(t[j - 1]) - truth) <= ((j + 1) * EPS[dn] + n * EPS['f64']) * truth, j    # + the cast
    # moments=None: a scalar, the trace
    t0 = S().trapprox(lambda x: x * lam_d, [n], dtype=DT[dn], device=dev)
    assert t0.dim() == 0 and abs(float(t0) - float(l64.sum())) <= (2 * EPS[dn] + n * EPS['f64']) * float(l64.sum())


@functools.lru_cache(maxsize=None)
def dense_spd():
    rng = np.random.default_rng(1)
    q = np.linalg.qr(rng.standard_normal((256, 256)))[0]
    ev = 1.0 / (1.0 + np.arange(256)) ** 2
    a = (q * ev) @ q.T
    return (a + a.T) / 2


def reference_algorithm(a, probes, moments, hutchpp, m):
    """the reference's trapprox (`stochastic.py:96-142`) restated with torch ops on the CPU in the dtype of `a`"""
    t = torch.zeros(moments, dtype=a.dtype)
    if hutchpp:
        s, g = probes[:m], probes[m:].clone()
        q = torch.linalg.qr((a @ s.T))[0].T
        z = torch.stack([torch.stack([q[j].dot(g[k]) for k in range(m)]) for j in range(m)])
        g = g - z.T @ q
        mq, mg = q, g
        for j in range(moments):
            mq, mg = mq @ a.T, mg @ a.T
            t[j] = sum(q[i].dot(mq[i]) for i in range(m)) + sum(g[i].dot(mg[i]) for i in range(m)) / m
        return t
    for v in probes:
        mv = v
        for j in range(moments):
            mv = a @ mv
            t[j] += mv.dot(v)
    return t / len(probes)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('method', ['rademacher', 'gaussian'])
@pytest.mark.parametrize('hutchpp', [False, True])
def test_trapprox_dense_against_the_model_on_the_same_probes(dev, dn, method, hutchpp):
    a64, N, moments, samples = dense_spd(), 256, 3, 12
    m = 4 if hutchpp else samples
    a = torch.as_tensor(a64, dtype=DT[dn])
    got = f64(S().trapprox(a.to(dev), moments=moments, samples=samples, method=method, hutchpp=hutchpp, generator=gen(21)))
    seed = seed_of(21)
    a_dn = a.double().numpy()                                   # the matrix the backend sees
    if hutchpp:
        p64 = R.probes(method, seed, 2 * m, N)
        truth = R.hutchpp(a_dn, p64[:m], p64[m:], moments)
    else:
        p64 = R.probes(method, seed, samples, N)
        truth = R.hutchinson(a_dn, p64, moments)
    ref = reference_algorithm(a, torch.as_tensor(p64, dtype=DT[dn]), moments, hutchpp, m).double().numpy()
    err, err_ref = np.abs(got - truth), np.abs(ref - truth)
    bound = 2 * err_ref + 4 * m * N * EPS[dn] * np.abs(truth)
    print(f'dense {dn} {method} hutchpp={hutchpp}: err {err}, reference {err_ref}, fraction {(err / bound).max():.2e}')
    assert (err <= bound).all(), (err, bound)
    # and it is an estimate of the trace
    assert abs(got[0] - np.trace(a64)) <= 0.5 * np.trace(a64)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_hutchpp_is_exact_on_a_rank_3_matrix_and_drops_the_fourth_column(dev, dn):
    N = 256
    b = np.random.default_rng(2).standard_normal((N, 3))
    a = torch.as_tensor(b @ b.T, dtype=DT[dn], device=dev)
    tr = float(np.trace(f64(a)))
    # The estimate is exact whatever the sketch.  Whether the fourth column DROPS depends on the first three:
    # rounding noise along q_j is amplified by |y_j| / |y_j minus its projection| (an ill-conditioned sketch
    # leaves a residual above 64 eps in the fourth column, which is then kept as a harmless unit vector of
    # noise).  So the drop is asserted on the first generator seed whose sketch, in the float64 model, keeps
    # every independent column at more than a tenth of its length: an amplification below 10 against the 64.
    for sd in range(5, 64):
        y = f64(a) @ R.probes('rademacher', seed_of(sd), 4, N).T
        r = np.abs(np.diag(np.linalg.qr(y)[1]))
        if (r[:3] >= 0.1 * np.linalg.norm(y, axis=0)[:3]).all():
            break
    t = float(S().trapprox(a, samples=12, hutchpp=True, generator=gen(sd)))
    print(f'rank 3 {dn} (generator seed {sd}): relative error {abs(t - tr) / tr:.2e}')
    assert abs(t - tr) <= 64 * N * EPS[dn] * tr
    t5 = float(S().trapprox(a, samples=12, hutchpp=True, generator=gen(5)))     # an ill-conditioned sketch
    assert abs(t5 - tr) <= 64 * N * EPS[dn] * tr
    # the drop rule, seen directly: A S has rank 3
    s = S()._fill(torch.empty(4, N, dtype=DT[dn], device=dev), L().STOCH_RADEMACHER, seed_of(sd))
    q = (a @ s.T).T.contiguous()
    S()._orth(q)
    assert [float(q[j].abs().max()) > 0 for j in range(4)] == [True, True, True, False]


@pytest.mark.parametrize('hutchpp', [False, True])
def test_trapprox_same_seed_same_bits(dev, hutchpp):
    n = 1027
    lam = torch.linspace(0.1, 2, n, device=dev)

    def mv(x):
        return x * lam + x.roll(1) * 0.1 + x.roll(-1) * 0.1
    kw = dict(moments=3, samples=7, method='gaussian', hutchpp=hutchpp, device=dev)
    torch.manual_seed(11)
    a = S().trapprox(mv, [n], **kw)
    torch.manual_seed(11)
    b = S().trapprox(mv, [n], **kw)
    c = S().trapprox(mv, [n], **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a, S().trapprox(mv, [n], generator=gen(3), **kw)) is False
    assert torch.equal(S().trapprox(mv, [n], generator=gen(3), **kw), S().trapprox(mv, [n], generator=gen(3), **kw))


@pytest.mark.parametrize('hutchpp', [False, True])
def test_trapprox_captures_in_a_graph(dev, hutchpp):
    n = 1027
    lam = torch.linspace(0.1, 2, n, device=dev)

    def mv(x):
        return x * lam
    kw = dict(moments=3, samples=6, hutchpp=hutchpp, device=dev)
    eager = S().trapprox(mv, [n], generator=gen(8), **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = S().trapprox(mv, [n], generator=gen(8), **kw)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    g.replay()                                               # a replay reuses the captured seed
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ----------------------------------------------------------------------------------- maxeig_power
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_maxeig_power(dev, dn):
    n = 1027
    lam = torch.rand(n, generator=gen(1), dtype=torch.float64) * 0.4 + 0.1
    lam[17] = 1.0
    lam = lam.to(DT[dn]).to(dev)
    calls = [0]

    def mv(x):
        calls[0] += 1
        return x * lam
    res = {}
    for ce in (1, 8, 64):
        calls[0] = 0
        res[ce] = S().maxeig_power(mv, [n], check_every=ce, generator=gen(4), dtype=DT[dn], device=dev)
        res[ce, 'calls'] = calls[0]
    mu = res[8]
    assert mu.dim() == 0 and mu.dtype == DT[dn] and mu.device.type == 'cuda'
    assert abs(float(mu) - 1) <= 1e-6 + 8 * EPS[dn]
    assert torch.equal(res[1], res[8]) and torch.equal(res[1], res[64])
    assert res[1, 'calls'] <= res[8, 'calls'] <= res[1, 'calls'] + 7 and res[64, 'calls'] % 64 == 0
    # the numpy model on the same probe stops at the same estimate
    v0 = R.rademacher(seed_of(4), 0, n)
    model = R.power_iteration(np.diag(f64(lam)), v0)
    assert abs(float(mu) - model) <= 1e-6 + 8 * EPS[dn]
    # a tensor operator (dense and sparse), default backend from the tensor
    a = torch.diag(lam)
    assert abs(float(S().maxeig_power(a)) - 1) <= 1e-6 + 8 * EPS[dn]
    assert abs(float(S().maxeig_power(a.to_sparse())) - 1) <= 1e-6 + 8 * EPS[dn]


# ------------------------------------------------------------------------------------------ vbald
def golden_spectrum(name, n):
    i = np.arange(n, dtype=np.float64)
    return {'linear': np.linspace(0.2, 1.0, n), 'sqrt': 0.1 + 0.9 * np.sqrt((i + 0.5) / n)}[name]


def test_vbald_runs_without_upper_in_float64(dev):
    """the reference raises here on the CPU (it drops the backend on the way to maxeig_power: quirk Q50)"""
    n = 4096
    lam = torch.as_tensor(golden_spectrum('linear', n), device=dev)
    torch.manual_seed(0)
    ld = S().vbald(lambda x: x * lam, [n], dtype=torch.float64, device=dev)
    assert ld.dim() == 0 and ld.dtype == torch.float64 and ld.device.type == 'cuda'
    truth = float(lam.log().sum())
    assert math.isfinite(float(ld)) and abs(float(ld) - truth) <= abs(truth)     # the right order of magnitude


@pytest.mark.parametrize('name', ['linear', 'sqrt'])
def test_vbald_within_the_reference_spread(dev, name):
    """the same algorithm with the same 64-node noise: the median |relative error| of 20 seeded runs is at most
    the 75th percentile of the 20 the reference recorded (tests/golden/stochastic_vbald.json)"""
    gold = json.load(open(os.path.join(GOLDEN, 'stochastic_vbald.json')))
    n = gold['n']
    lam64 = golden_spectrum(name, n)
    lam = torch.as_tensor(lam64, dtype=torch.float32)
    truth = gold['spectra'][name]['truth_logdet']
    assert abs(truth - float(np.log(lam64).sum())) <= 1e-9 * abs(truth)
    lam_d = lam.to(dev)
    errs = []
    for run in range(gold['runs']):
        torch.manual_seed(2000 + run)
        ld = float(S().vbald(lambda x: x * lam_d, [n], upper=float(lam.max()), device=dev))
        errs.append(abs(ld - truth) / abs(truth))
    assert np.isfinite(errs).all()
    p75 = float(np.percentile(np.abs(gold['spectra'][name]['reference_rel_err']), 75))
    print(f'vbald {name}: median |rel err| {np.median(errs):.3f}, reference median '
          f'{np.median(np.abs(gold["spectra"][name]["reference_rel_err"])):.3f}, p75 {p75:.3f}')
    assert np.median(errs) <= p75
