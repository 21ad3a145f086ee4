"""`sugar` on the GPU: golden parity of every function, the per-record backward error of `lmdiv` on the graded
families of tests/_solver_ref.py (its measure `solve_eta` and its bound `eta_bound`, per column of every record,
no record left out), row exchanges, layouts read in place, column blocks, `rmdiv`, the Cholesky contract (lower
triangle only, NaN records), `inv('chol')`, autograd and graph capture.

The reference of the bounds is torch on the CPU in the same dtype: `torch.linalg.solve` for 'lu',
`torch.linalg.cholesky` + `torch.cholesky_solve` for 'chol' (what the reference's `lmdiv` runs)."""
import os
import numpy as np
import pytest
import torch
from conftest import GOLDEN, TOL, relerr
import _solver_ref as R
import _lstsq_ref as Q

pytestmark = pytest.mark.gpu
DNS = ['f32', 'f64']
TT = {'f32': torch.float32, 'f64': torch.float64}
ORDERS = tuple(range(1, 9))
KS = (1, 3, 8)


def S():
    from nitorch_fastmath_amd import sugar
    return sugar


def t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)


def c(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'sugar.npz'))


def cpu_ref(a, b, method):
    a, b = torch.from_numpy(np.array(a)), torch.from_numpy(np.array(b))
    if method == 'lu':
        return torch.linalg.solve(a, b).numpy()
    return torch.cholesky_solve(b, torch.linalg.cholesky(a, upper=False), upper=False).numpy()


def column_excess(a, got, ref, b, N, dn, what, keep=None):
    """solve_eta / eta_bound of every column of every record; every record has a verdict"""
    worst = 0.0
    for col in range(b.shape[-1]):
        eta = R.solve_eta(a, got[..., col], b[..., col], dn)
        eref = R.solve_eta(a, ref[..., col], b[..., col], dn)
        ex = eta / R.eta_bound(eref, N, dn)
        if keep is not None:
            ex = ex[keep]
        assert not np.isnan(ex).any(), what
        w, i = R.worst(ex)
        print(f'{what} col {col}: worst eta / bound = {w:.3g} (record {i}), worst reference eta / (N eps) = '
              f'{np.max(eref[np.isfinite(eref)]) / (N * R.EPS[dn]):.3g}')
        assert w <= 1.0, (what, col, f'record {i}: {w:.3g} times its bound')
        worst = max(worst, w)
    return worst


def rhs(n, N, K, dn, seed):
    return np.random.default_rng(seed).standard_normal((n, N, K)).astype(R.NP[dn])


# ------------------------------------------------------------------------------------------------ golden parity
@pytest.mark.parametrize('dn', DNS)
def test_golden_parity(dev, golden, dn):
    """kernel-backed (N <= 8) and torch-routed (N = 12, svd, pinv) functions against the reference's results"""
    s = S()
    for N in ORDERS + (12,):
        def G(k):
            return golden[f'{dn}_{N}_{k}']
        a, spd, b, v, w, ar = (t(G(k), dev) for k in ('a', 'spd', 'b', 'v', 'w', 'ar'))
        got = {'lmdiv_lu': s.lmdiv(a, b), 'lmdiv_chol': s.lmdiv(spd, b, 'chol'), 'lmdiv_svd': s.lmdiv(a, b, 'svd'),
               'lmdiv_pinv': s.lmdiv(a, b, 'pinv'), 'inv_lu': s.inv(a), 'inv_chol': s.inv(spd, 'chol'),
               'inv_svd': s.inv(a, 'svd'), 'inv_pinv': s.inv(a, 'pinv'), 'solvevec': s.solvevec(a, v),
               'kron2': s.kron2(a[0], b[0]), 'outer': s.outer(v, w), 'trace': s.trace(a), 'dot': s.dot(v, b[..., 0]),
               'mdot': s.mdot(a, spd), 'round': s.round(a, 2), 'rmdiv': s.rmdiv(ar, a),
               'inv_chol_2d': s.inv(spd[0], 'chol')}
        for k, x in got.items():
            ref = G(k)
            assert tuple(x.shape) == ref.shape and x.dtype == TT[dn], (N, k)
            assert relerr(c(x), ref) <= TOL[dn], (N, k, relerr(c(x), ref))
        assert relerr(c(s.matvec(a, v)), np.einsum('nij,nj->ni', G('a').astype(np.float64), G('v').astype(np.float64))) <= TOL[dn]
        assert s.trace(a, keepdim=True).shape == (16, 1, 1) and s.dot(v, v, keepdim=True).shape == (16, 1)
    q = torch.eye(5, dtype=TT[dn], device=dev)[[3, 0, 4, 1, 2]]          # exact in both dtypes
    ok, m = s.is_orthonormal(q, return_matrix=True)
    assert ok is True and m.shape == (5, 5) and s.is_orthonormal(2 * q) is False
    # out= and the reference's reading of `method`
    a, b = t(golden[f'{dn}_4_a'], dev), t(golden[f'{dn}_4_b'], dev)
    o = torch.empty_like(b)
    assert s.lmdiv(a, b, 'LU', out=o) is o and relerr(c(o), golden[f'{dn}_4_lmdiv_lu']) <= TOL[dn]
    with pytest.raises(RuntimeError, match='out='):
        s.lmdiv(a.clone().requires_grad_(), b, out=o)


# ------------------------------------------------------------------------------------------------ per-record accuracy
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', ORDERS)
def test_lmdiv_graded_per_record(dev, dn, N):
    """general_graded ('lu') and the full form of spd_graded ('chol'), every cond, n = 209 and 17, K = 1, 3, 8,
    every record times its own power of two: eta <= 2 eta_ref + 4 N eps for every column of every record."""
    s = S()
    for cond in R.CONDS[dn]:
        for n in R.NS:
            k = R.pow2_scales(n, R.KMAX_LINEAR[dn], 900 + N)
            gen = R.scaled(R.general_graded(n, N, cond, dn, 200 + N)[0], k)
            spd = R.scaled(R.to_full(R.spd_graded(n, N, cond, dn, 100 + N)[0]).astype(R.NP[dn]), k)
            for K in KS:
                b = rhs(n, N, K, dn, 910 + K)
                for method, a in (('lu', gen), ('chol', spd)):
                    got = c(s.lmdiv(t(a, dev), t(b, dev), method))
                    ref = cpu_ref(a, b, method)
                    assert got.shape == (n, N, K) and np.isfinite(ref).all(), (method, cond, n, K)
                    column_excess(a, got, ref, b, N, dn, f'{method} N={N} {dn} cond={cond:g} n={n} K={K}')
                if K == 1:
                    x = c(s.solvevec(t(gen, dev), t(b[..., 0], dev)))
                    assert np.array_equal(x, c(s.lmdiv(t(gen, dev), t(b, dev)))[..., 0])


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', [3, 4, 8])
def test_row_exchanges(dev, dn, N):
    """zero and tiny leading entries: the same bound on the records the CPU reference solves finitely"""
    rng = np.random.default_rng(40 + N)
    n = 2000
    a = rng.standard_normal((n, N, N))
    a[:, 0, 0] = 0.0
    a[::3, 1, 1] = 1e-300
    a = (a + 0.0).astype(R.NP[dn])
    b = rhs(n, N, 3, dn, 41)
    ref = cpu_ref(a, b, 'lu')
    keep = np.isfinite(ref).all((1, 2))
    assert keep.sum() >= 0.99 * n
    got = c(S().lmdiv(t(a, dev), t(b, dev)))
    column_excess(a, got, ref, b, N, dn, f'row exchanges N={N} {dn}', keep)


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', [3, 6, 8])
def test_layouts_read_in_place(dev, dn, N):
    s = S()
    rng = np.random.default_rng(50 + N)
    K, n = 3, 3001
    a = (rng.standard_normal((n, N, N)) + 6 * np.eye(N)).astype(R.NP[dn])
    b = rhs(n, N, K, dn, 51)
    ad, bd = t(a, dev), t(b, dev)
    base = s.lmdiv(ad, bd)
    ref = cpu_ref(a, b, 'lu')
    column_excess(a, c(base), ref, b, N, dn, f'contiguous N={N} {dn}')
    # batches of 1, 65 and 3001 give the same records
    for m in (1, 65):
        assert torch.equal(s.lmdiv(ad[:m].clone(), bd[:m].clone()), base[:m]), m
    def same(x, what, rows=slice(None)):
        """another kernel variant of the same arithmetic: the same bound (instruction selection may differ by an
        ulp between variants: measured, float32 orders 6 and 8)"""
        x = c(x).reshape(-1, N, K)
        print(f'{what} N={N} {dn}: max |x - contiguous| / max |x| = {relerr(x, c(base[rows])):.3g}')
        column_excess(a[rows], x, ref[rows], b[rows], N, dn, f'{what} N={N} {dn}')

    # a.mT of a contiguous tensor
    at = t(a.transpose(0, 2, 1).copy(), dev).mT
    assert not at.is_contiguous() or N == 1
    same(s.lmdiv(at, bd), 'a.mT')
    # channel-first a, b and result
    n2 = 3000
    cf = (lambda x: x[:n2].reshape(40, 75, *x.shape[1:]).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    acf, bcf = cf(ad), cf(bd)
    assert acf.stride(1) == 1 and bcf.stride(1) == 1
    xcf = s.lmdiv(acf, bcf)
    assert xcf.stride() == bcf.stride()                     # the layout of b is handed on
    same(xcf, 'channel-first', slice(0, n2))
    # one a against 2000 b, one b against 2000 a
    x1 = s.lmdiv(ad[7], bd[:2000])
    assert x1.shape == (2000, N, K)
    column_excess(np.broadcast_to(a[7], (2000, N, N)), c(x1), cpu_ref(np.broadcast_to(a[7], (2000, N, N)), b[:2000], 'lu'),
                  b[:2000], N, dn, f'one a N={N} {dn}')
    x2 = s.lmdiv(ad[:2000], bd[7])
    assert x2.shape == (2000, N, K)
    b7 = np.broadcast_to(b[7], (2000, N, K))
    column_excess(a[:2000], c(x2), cpu_ref(a[:2000], b7, 'lu'), b7, N, dn, f'one b N={N} {dn}')
    # out= aliasing b
    b2 = bd.clone()
    assert s.lmdiv(ad, b2, out=b2) is b2 and torch.equal(b2, base)
    # K = 11: column blocks on views of b and of the result, bit for bit the separate calls on the same views
    b11 = t(rhs(n, N, 11, dn, 52), dev)
    x11 = s.lmdiv(ad, b11)
    cap = s.max_cols(TT[dn], N)
    assert x11.shape == (n, N, 11) and x11.is_contiguous() and cap < 11
    for c0 in range(0, 11, cap):
        assert torch.equal(x11[..., c0:c0 + cap], s.lmdiv(ad, b11[..., c0:c0 + cap])), c0


# ------------------------------------------------------------------------------------------------ column blocks
# (family, method, rows, K per dtype): the smallest systems at which every family's column cap is below K
BLOCK_CASES = [('lu', 'lu', 8, {'f64': 8, 'f32': 11}), ('chol', 'chol', 8, {'f64': 8, 'f32': 11}),
               ('svd', 'svd', 8, {'f64': 8, 'f32': 11}), ('lstsq', 'pinv', 12, {'f64': 6, 'f32': 11})]


def block_bound(family, a, got, b, dn, what):
    """the family's per-record bound on one block of columns: `column_excess` against torch on the CPU in the
    dtype (lu, chol, and the reference's svd composition), tests/_lstsq_ref.py's `excess` for the tall systems"""
    if family == 'lstsq':
        assert Q.excess(got, a, b, dn, what=what).max() <= 1.0, what
        return
    if family == 'svd':
        u, sv, v = torch.svd(torch.from_numpy(np.array(a)))
        ref = torch.matmul(v, u.transpose(-1, -2).matmul(torch.from_numpy(np.array(b))) / sv[..., None]).numpy()
    else:
        ref = cpu_ref(a, b, family)
    column_excess(a, got, ref, b, a.shape[-1], dn, what)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('case', BLOCK_CASES, ids=[case[0] for case in BLOCK_CASES])
def test_column_blocks_are_the_separate_calls(dev, dn, case, monkeypatch):
    """More columns than one launch takes, 130 records, every family: the result is bit for bit that of one call
    per block of columns into the same view of a buffer of the same layout (the same kernel variant on both
    sides), with a plain b, and with one broadcast a and out= a transposed view of a larger buffer; every block
    meets the family's per-record bound."""
    s = S()
    family, method, M, ks = case
    N, n, k = 8, 130, ks[dn]
    cap = {'lu': lambda: s.max_cols(TT[dn], N), 'chol': lambda: s.max_cols(TT[dn], N),
           'svd': lambda: s.svd_max_cols(TT[dn], M, N), 'lstsq': lambda: s.lstsq_max_cols(TT[dn], N)}[family]()
    blocks = [(c0, min(c0 + cap, k)) for c0 in range(0, k, cap)]
    assert 1 <= cap < k and len(blocks) == 2
    rng = np.random.default_rng(300 + M)
    g = rng.standard_normal((n, M, N))
    if family == 'chol':
        g = g @ g.transpose(0, 2, 1) + N * np.eye(N)
    elif family != 'lstsq':
        g = g + 6 * np.eye(N)
    a = g.astype(R.NP[dn])
    b = rng.standard_normal((n, M, k)).astype(R.NP[dn])
    ad, bd = t(a, dev), t(b, dev)
    launches = []
    launch = s._launch
    monkeypatch.setattr(s, '_launch', lambda *args: (launches.append(args[-1].shape[-1]), launch(*args))[1])

    def check(a_np, a_dev, got, full, what):
        assert launches == [c1 - c0 for c0, c1 in blocks], (what, launches)
        assert full.stride() == got.stride() and got.shape == (n, N, k)
        for c0, c1 in blocks:
            assert s.lmdiv(a_dev, bd[..., c0:c1], method=method, out=full[..., c0:c1]).shape == (n, N, c1 - c0)
        assert torch.equal(got, full), what
        for c0, c1 in blocks:
            block_bound(family, a_np, c(got)[..., c0:c1], b[..., c0:c1], dn, f'{what} {family} {dn} columns {c0}:{c1}')

    got = s.lmdiv(ad, bd, method=method)
    assert got.is_contiguous()
    check(a, ad, got, torch.empty_like(got), 'plain b')
    # one a for every b, the result into a transposed view of a larger buffer
    del launches[:]
    view = (lambda: torch.zeros(n + 3, k + 2, N + 1, dtype=TT[dn], device=dev)[:n, :k, :N].transpose(-1, -2))
    out = view()
    assert s.lmdiv(ad[:1], bd, method=method, out=out) is out and not out.is_contiguous()
    check(np.broadcast_to(a[:1], a.shape), ad[:1], out, view(), 'broadcast a, out= a transposed view')


@pytest.mark.parametrize('dn', DNS)
def test_order_12_takes_the_torch_route(dev, dn):
    rng = np.random.default_rng(60)
    a = (rng.standard_normal((65, 12, 12)) + 8 * np.eye(12)).astype(R.NP[dn])
    b = rhs(65, 12, 3, dn, 61)
    x = np.linalg.solve(a.astype(np.float64), b.astype(np.float64))
    assert relerr(c(S().lmdiv(t(a, dev), t(b, dev))), x) <= TOL[dn]
    spd = (a @ a.transpose(0, 2, 1) / 12 + np.eye(12)).astype(R.NP[dn])
    xs = np.linalg.solve(spd.astype(np.float64), b.astype(np.float64))
    assert relerr(c(S().lmdiv(t(spd, dev), t(b, dev), 'chol')), xs) <= TOL[dn]


# ------------------------------------------------------------------------------------------------ rmdiv
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('k', [1, 3, 5])
def test_rmdiv_is_a_times_inverse_b(dev, dn, k):
    """X = A B^-1 for a (n, k, 4), b (n, 4, 4): X b = a, held to the eta bound on the transposed system
    b^T X^T = a^T (reference: torch.linalg.solve on the CPU)"""
    m, n = 4, 209
    rng = np.random.default_rng(70 + k)
    bm = R.general_graded(n, m, R.CONDS[dn][1], dn, 71)[0]
    a = rng.standard_normal((n, k, m)).astype(R.NP[dn])
    x = S().rmdiv(t(a, dev), t(bm, dev))
    assert x.shape == (n, k, m) and x.is_contiguous()
    bt, at = bm.transpose(0, 2, 1).copy(), a.transpose(0, 2, 1).copy()
    column_excess(bt, c(x).transpose(0, 2, 1), cpu_ref(bt, at, 'lu'), at, m, dn, f'rmdiv k={k} {dn}')
    o = torch.empty_like(x)
    assert S().rmdiv(t(a, dev), t(bm, dev), out=o) is o and torch.equal(o, x)


# ------------------------------------------------------------------------------------------------ chol
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', [2, 5, 8])
def test_chol_reads_the_lower_triangle_only(dev, dn, N):
    n = 130
    spd = R.to_full(R.spd_graded(n, N, R.CONDS[dn][0], dn, 100 + N)[0]).astype(R.NP[dn])
    b = rhs(n, N, 3, dn, 80)
    clean = S().lmdiv(t(spd, dev), t(b, dev), 'chol')
    junk = spd.copy()
    iu = np.triu_indices(N, 1)
    junk[:, iu[0], iu[1]] = np.random.default_rng(81).standard_normal((n, len(iu[0]))).astype(R.NP[dn]) * 1e3
    assert torch.equal(S().lmdiv(t(junk, dev), t(b, dev), 'chol'), clean) and torch.isfinite(clean).all()
    assert torch.equal(S().inv(t(junk, dev), 'chol'), S().inv(t(spd, dev), 'chol'))


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('pos', [0, 63, 64, 129])
def test_chol_indefinite_record_is_nan_and_alone(dev, dn, pos):
    N, n = 5, 130
    spd = R.to_full(R.spd_graded(n, N, R.CONDS[dn][0], dn, 100 + N)[0]).astype(R.NP[dn])
    b = rhs(n, N, 3, dn, 82)
    clean = S().lmdiv(t(spd, dev), t(b, dev), 'chol')
    bad = spd.copy()
    bad[pos] = R.to_full(R.indefinite(1, N, dn, 83))[0].astype(R.NP[dn])
    for fn in (lambda m: S().lmdiv(t(m, dev), t(b, dev), 'chol'), lambda m: S().inv(t(m, dev), 'chol')):
        got, ok = fn(bad), fn(spd)
        assert torch.isnan(got[pos]).all()
        rest = torch.arange(n, device=dev) != pos
        assert torch.equal(got[rest], ok[rest]) and torch.isfinite(ok).all()
    assert torch.equal(clean, S().lmdiv(t(spd, dev), t(b, dev), 'chol'))


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', ORDERS)
def test_inv_chol_identity_residual(dev, dn, N):
    for cond in R.CONDS[dn]:
        for n in R.NS:
            spd = R.to_full(R.spd_graded(n, N, cond, dn, 100 + N)[0]).astype(R.NP[dn])
            tr = R.Truth(spd, dn)
            ex = R.identity_excess(c(S().inv(t(spd, dev), 'chol')), tr)
            assert ex.shape == (n,) and not np.isnan(ex).any()
            w, i = R.worst(ex)
            print(f'inv chol N={N} {dn} cond={cond:g} n={n}: worst excess {w:.3g}')
            assert w <= 1.0, (cond, n, f'record {i}: {w:.3g} times its bound')


# ------------------------------------------------------------------------------------------------ autograd, graphs
def test_gradcheck(dev):
    s = S()
    g = torch.Generator(device='cpu').manual_seed(5)
    a = (torch.randn(5, 3, 3, dtype=torch.float64, generator=g) + 4 * torch.eye(3, dtype=torch.float64)).to(dev)
    b = torch.randn(5, 3, 2, dtype=torch.float64, generator=g).to(dev)
    r = torch.randn(5, 2, 3, dtype=torch.float64, generator=g).to(dev)
    v = torch.randn(5, 3, dtype=torch.float64, generator=g).to(dev)
    req = (lambda x: x.clone().requires_grad_())
    assert torch.autograd.gradcheck(s.lmdiv, (req(a), req(b)))
    assert torch.autograd.gradcheck(s.lmdiv, (req(a[0]), req(b)))            # one a, broadcast
    assert torch.autograd.gradcheck(s.lmdiv, (req(a), req(b[0])))            # one b, broadcast
    assert torch.autograd.gradcheck(s.rmdiv, (req(r), req(a)))
    assert torch.autograd.gradcheck(s.solvevec, (req(a), req(v)))
    spd = a @ a.mT
    assert torch.autograd.gradcheck(lambda x: s.lmdiv(spd, x, 'chol'), (req(b),))
    assert torch.autograd.gradcheck(lambda m, x: s.lmdiv(m @ m.mT, x, 'chol'), (req(a), req(b)))   # torch route


def test_graph_capture(dev):
    from nitorch_fastmath_amd import utils
    s = S()
    rng = np.random.default_rng(90)
    mk = (lambda: (t((rng.standard_normal((300, 4, 4)) + 5 * np.eye(4)).astype(np.float32), dev),
                   t(rng.standard_normal((300, 4, 3)).astype(np.float32), dev)))
    a0, b0 = mk()
    step = utils.graphed(lambda a, b: s.lmdiv(a, b), a0, b0)
    for _ in range(2):
        a1, b1 = mk()
        x = step(a1, b1).clone()
        assert torch.equal(x, s.lmdiv(a1, b1))
