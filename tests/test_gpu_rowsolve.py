"""Square solves of orders 9..16 on the GPU (`sugar.lmdiv` / `rmdiv` / `solvevec` / `inv('chol')` on the row-per-lane
kernels of `nfm_rowsolve`): the per-record backward error on the graded families of tests/_solver_ref.py (every
column of every record, no record left out), exact pivoting, layouts and tiles bit for bit, columns that do not depend
on their neighbours, bad records that stay alone, the public surface, autograd and graph capture.

The reference of the bounds is torch on the CPU in the same dtype (`cpu_ref` of tests/test_gpu_sugar.py):
`torch.linalg.solve` for 'lu', `torch.linalg.cholesky` + `torch.cholesky_solve` for 'chol'.  The bound is the
project's: eta <= 2 eta_ref + 4 N eps (`column_excess`).  The fixtures were checked on the CPU: the reference is
finite on every record of the graded families and of the `row exchanges` batches."""
import numpy as np
import pytest
import torch
import _solver_ref as R
from test_gpu_sugar import column_excess, cpu_ref, rhs, t, c

pytestmark = pytest.mark.gpu
DNS = ['f32', 'f64']
TT = {'f32': torch.float32, 'f64': torch.float64}
ORDERS = tuple(range(9, 17))
METHODS = ('lu', 'chol')
# the two forms of each dtype's table sit at the ends of the range; 12 / 13 is a tile of another pitch
EDGE_ORDERS = (9, 12, 16)


def S():
    from nitorch_fastmath_amd import sugar
    return sugar


def cap_of(dn, N):
    return S().rowsolve_max_cols(TT[dn], N)


def graded(method, n, N, cond, dn):
    """general_graded ('lu') or the full form of spd_graded ('chol'), every record times its own power of two"""
    k = R.pow2_scales(n, R.KMAX_LINEAR[dn], 900 + N)
    if method == 'lu':
        return R.scaled(R.general_graded(n, N, cond, dn, 200 + N)[0], k)
    return R.scaled(R.to_full(R.spd_graded(n, N, cond, dn, 100 + N)[0]).astype(R.NP[dn]), k)


def graded_cases(dn, N):
    """(method, cond, n, K, a, b) of the per-record accuracy test"""
    for cond in R.CONDS[dn]:
        for n in R.NS:
            for K in (1, 3, cap_of(dn, N)):
                b = rhs(n, N, K, dn, 910 + K)
                for method in METHODS:
                    yield method, cond, n, K, graded(method, n, N, cond, dn), b


def graded_worst(dev, dn, N):
    """worst eta / bound per method over `graded_cases` (asserted <= 1 for every column of every record)"""
    worst = {m: 0.0 for m in METHODS}
    for method, cond, n, K, a, b in graded_cases(dn, N):
        got = c(S().lmdiv(t(a, dev), t(b, dev), method))
        ref = cpu_ref(a, b, method)
        assert got.shape == (n, N, K) and np.isfinite(ref).all(), (method, cond, n, K)
        w = column_excess(a, got, ref, b, N, dn, f'{method} N={N} {dn} cond={cond:g} n={n} K={K}')
        worst[method] = max(worst[method], w)
    return worst


def spd_of(n, N, dn, seed=0):
    return R.to_full(R.spd_graded(n, N, R.CONDS[dn][0], dn, 100 + N + seed)[0]).astype(R.NP[dn])


def system(method, n, N, dn, seed):
    """a well conditioned batch for the bit-for-bit tests: randn + 6 I ('lu'), a graded SPD family ('chol')"""
    if method == 'chol':
        return spd_of(n, N, dn)
    return (np.random.default_rng(seed).standard_normal((n, N, N)) + 6 * np.eye(N)).astype(R.NP[dn])


# ------------------------------------------------------------------------------------------------ per-record accuracy
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', ORDERS)
def test_lmdiv_graded_per_record(dev, dn, N):
    """every cond, n = 209 and 17, K = 1, 3, cap, both methods: eta <= 2 eta_ref + 4 N eps for every column of every
    record (worst measured excess per (method, dtype, N): profiles/rowsolve_accuracy.md)"""
    graded_worst(dev, dn, N)


# ------------------------------------------------------------------------------------------------ pivoting
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', [9, 13, 16])
@pytest.mark.parametrize('perm', ['reversal', 'shift5'])
def test_permuted_scalings_are_exact(dev, dn, N, perm):
    """a = P D (P a permutation, D powers of two), b small integers: every step pivots from another lane and another
    slot, every multiplier is zero, and X = D^-1 P^T b is exact -- bit for bit."""
    n, K = 50, 3
    rng = np.random.default_rng(30 + N)
    col = (N - 1 - np.arange(N)) if perm == 'reversal' else (np.arange(N) + 5) % N      # a[i, col[i]] != 0
    d = np.ldexp(1.0, rng.integers(-8, 9, (n, N)))
    a = np.zeros((n, N, N))
    a[:, np.arange(N), col] = d[:, col] * np.where(rng.random((n, N)) < 0.5, -1.0, 1.0)
    b = rng.integers(-8, 9, (n, N, K)).astype(np.float64)
    x = np.zeros((n, N, K))
    x[:, col, :] = b / a[:, np.arange(N), col][..., None]                               # row i: a[i, col] x[col] = b[i]
    assert np.array_equal(np.einsum('nij,njk->nik', a, x), b)
    a, b = a.astype(R.NP[dn]), b.astype(R.NP[dn])
    got = c(S().lmdiv(t(a, dev), t(b, dev)))
    assert got.dtype == R.NP[dn] and np.array_equal(got, x.astype(R.NP[dn]))
    v = c(S().solvevec(t(a, dev), t(b[..., 0], dev)))
    assert np.array_equal(v, x[..., 0].astype(R.NP[dn]))


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', EDGE_ORDERS)
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


# ------------------------------------------------------------------------------------------------ layouts and tiles
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', EDGE_ORDERS)
@pytest.mark.parametrize('method', METHODS)
def test_layouts_and_tiles_give_the_same_bits(dev, dn, N, method):
    s = S()
    K, n = 3, 3001
    a = system(method, n, N, dn, 50 + N)
    b = rhs(n, N, K, dn, 51)
    ad, bd = t(a, dev), t(b, dev)
    base = s.lmdiv(ad, bd, method)
    assert base.shape == (n, N, K) and base.is_contiguous()
    column_excess(a, c(base), cpu_ref(a, b, method), b, N, dn, f'contiguous {method} N={N} {dn}')
    # ragged and whole tiles
    for m in (1, 15, 16, 17, 65):
        assert torch.equal(s.lmdiv(ad[:m].clone(), bd[:m].clone(), method), base[:m]), m
    # a.mT of a contiguous tensor
    at = t(a.transpose(0, 2, 1).copy(), dev).mT
    assert not at.is_contiguous()
    assert torch.equal(s.lmdiv(at, bd, method), base)
    # channel-first a, b and result
    n2 = 3000
    cf = (lambda x: x[:n2].reshape(40, 75, *x.shape[1:]).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    acf, bcf = cf(ad), cf(bd)
    assert acf.stride(1) == 1 and bcf.stride(1) == 1
    xcf = s.lmdiv(acf, bcf, method)
    assert xcf.stride() == bcf.stride()                     # the layout of b is handed on
    assert torch.equal(xcf.reshape(n2, N, K), base[:n2])
    # one a against 2000 b, one b against 2000 a
    x1 = s.lmdiv(ad[7], bd[:2000], method)
    assert x1.shape == (2000, N, K) and torch.equal(x1, s.lmdiv(ad[7].expand(2000, N, N).contiguous(), bd[:2000], method))
    assert torch.equal(x1[7], base[7])
    x2 = s.lmdiv(ad[:2000], bd[7], method)
    assert x2.shape == (2000, N, K) and torch.equal(x2, s.lmdiv(ad[:2000], bd[7].expand(2000, N, K).contiguous(), method))
    assert torch.equal(x2[7], base[7])
    # out= aliasing b
    b2 = bd.clone()
    assert s.lmdiv(ad, b2, method, out=b2) is b2 and torch.equal(b2, base)
    # a base that is not 16-byte aligned
    if dn == 'f32' and N == 9:
        a1, b1 = ad[1:], bd[1:]
        assert a1.data_ptr() % 16 and b1.data_ptr() % 16 and a1.is_contiguous()
        assert torch.equal(s.lmdiv(a1, b1, method), base[1:])


# ------------------------------------------------------------------------------------------------ columns
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', EDGE_ORDERS)
@pytest.mark.parametrize('method', METHODS)
def test_a_column_does_not_depend_on_the_others(dev, dn, N, method):
    """column j of a K-wide call is `solvevec` on column j, bit for bit, for every K up to the cap (contiguous and
    strided right-hand sides); K = cap + 3 is the separate calls on the same views"""
    s = S()
    n, cap = 130, cap_of(dn, N)
    a = system(method, n, N, dn, 60 + N)
    b = rhs(n, N, cap + 3, dn, 61)
    ad, bd = t(a, dev), t(b, dev)
    cols = [s.solvevec(ad, bd[..., j].contiguous(), method) for j in range(cap + 3)]
    ref = cpu_ref(a, b, method)
    column_excess(a, c(torch.stack(cols, -1)), ref, b, N, dn, f'solvevec {method} N={N} {dn}')
    for K in range(1, cap + 1):
        for bk in (bd[..., :K], bd[..., :K].contiguous()):
            x = s.lmdiv(ad, bk, method)
            assert x.shape == (n, N, K)
            for j in range(K):
                assert torch.equal(x[..., j], cols[j]), (K, j, bk.is_contiguous())
    wide = s.lmdiv(ad, bd, method)
    assert wide.shape == (n, N, cap + 3) and wide.is_contiguous()
    full = torch.empty_like(wide)
    for c0, c1 in ((0, cap), (cap, cap + 3)):
        s.lmdiv(ad, bd[..., c0:c1], method, out=full[..., c0:c1])
    assert torch.equal(wide, full)
    for j in range(cap + 3):
        assert torch.equal(wide[..., j], cols[j]), j


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('pos', [0, 15, 16, 63, 64, 129])
def test_a_bad_record_stays_alone(dev, dn, pos):
    """130 records, one bad one: a zero row ('lu'), an indefinite matrix ('chol'), a NaN entry (both).  The bad record
    is non-finite -- NaN throughout for 'chol' --, every other record has the bits of the batch without it."""
    s = S()
    n, K = 130, 3
    rest = torch.arange(n, device=dev) != pos
    for N in (9, 16):
        b = t(rhs(n, N, K, dn, 82), dev)
        for method in METHODS:
            good = system(method, n, N, dn, 70 + N)
            clean = s.lmdiv(t(good, dev), b, method)
            assert torch.isfinite(clean).all()
            bads = []
            nan = good.copy()
            nan[pos, N - 2, 1] = np.nan                     # below the diagonal: 'chol' reads it
            bads.append(('nan', nan))
            if method == 'lu':
                zero = good.copy()
                zero[pos, N // 2, :] = 0.0
                bads.append(('zero row', zero))
            else:
                ind = good.copy()
                ind[pos] = R.to_full(R.indefinite(1, N, dn, 83))[0].astype(R.NP[dn])
                bads.append(('indefinite', ind))
            for what, bad in bads:
                got = s.lmdiv(t(bad, dev), b, method)
                assert not torch.isfinite(got[pos]).all(), (N, method, what)
                if method == 'chol':
                    assert torch.isnan(got[pos]).all(), (N, what)
                    inv = s.inv(t(bad, dev), 'chol')
                    assert torch.isnan(inv[pos]).all() and torch.equal(inv[rest], s.inv(t(good, dev), 'chol')[rest])
                assert torch.equal(got[rest], clean[rest]), (N, method, what)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', EDGE_ORDERS)
def test_chol_reads_the_lower_triangle_only(dev, dn, N):
    n = 130
    spd = spd_of(n, N, dn)
    b = t(rhs(n, N, 3, dn, 80), dev)
    clean = S().lmdiv(t(spd, dev), b, 'chol')
    junk = spd.copy()
    iu = np.triu_indices(N, 1)
    junk[:, iu[0], iu[1]] = np.nan
    assert torch.equal(S().lmdiv(t(junk, dev), b, 'chol'), clean) and torch.isfinite(clean).all()
    assert torch.equal(S().inv(t(junk, dev), 'chol'), S().inv(t(spd, dev), 'chol'))


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('k', [1, 5])
def test_rmdiv_is_a_times_inverse_b(dev, dn, k):
    """X = A B^-1 for a (n, k, 12), b (n, 12, 12): the eta bound on the transposed system b^T X^T = a^T"""
    m, n = 12, 209
    rng = np.random.default_rng(70 + k)
    bm = R.general_graded(n, m, R.CONDS[dn][1], dn, 71)[0]
    a = rng.standard_normal((n, k, m)).astype(R.NP[dn])
    x = S().rmdiv(t(a, dev), t(bm, dev))
    assert x.shape == (n, k, m) and x.is_contiguous()
    bt, at = bm.transpose(0, 2, 1).copy(), a.transpose(0, 2, 1).copy()
    column_excess(bt, c(x).transpose(0, 2, 1), cpu_ref(bt, at, 'lu'), at, m, dn, f'rmdiv k={k} {dn}')
    o = torch.empty_like(x)
    assert S().rmdiv(t(a, dev), t(bm, dev), out=o) is o and torch.equal(o, x)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', [9, 16])
def test_inv_chol(dev, dn, N):
    """A inv = I to `identity_bound` per record at every cond, and the bits of `lmdiv` against an explicit identity"""
    s = S()
    for cond in R.CONDS[dn]:
        for n in R.NS:
            spd = R.to_full(R.spd_graded(n, N, cond, dn, 100 + N)[0]).astype(R.NP[dn])
            inv = s.inv(t(spd, dev), 'chol')
            ex = R.identity_excess(c(inv), R.Truth(spd, dn))
            assert ex.shape == (n,) and not np.isnan(ex).any()
            w, i = R.worst(ex)
            print(f'inv chol N={N} {dn} cond={cond:g} n={n}: worst excess {w:.3g}')
            assert w <= 1.0, (cond, n, f'record {i}: {w:.3g} times its bound')
            eye = torch.eye(N, dtype=TT[dn], device=dev)
            assert torch.equal(inv, s.lmdiv(t(spd, dev), eye, 'chol'))
    assert torch.equal(s.inv(t(spd[0], dev), 'chol'), inv[0])                # a single matrix


@pytest.mark.parametrize('dn', DNS)
def test_out_is_honoured(dev, dn):
    s = S()
    N, n = 12, 65
    a, spd = t(system('lu', n, N, dn, 90), dev), t(spd_of(n, N, dn), dev)
    b, v, r = t(rhs(n, N, 3, dn, 91), dev), t(rhs(n, N, 1, dn, 92)[..., 0], dev), t(rhs(n, N, 2, dn, 93), dev).mT
    for method, m in (('lu', a), ('chol', spd)):
        o = torch.empty_like(b)
        assert s.lmdiv(m, b, method, out=o) is o and torch.equal(o, s.lmdiv(m, b, method))
        o = torch.empty_like(v)
        x = s.solvevec(m, v, method, out=o)                  # a view of o with its shape
        assert x.data_ptr() == o.data_ptr() and x.shape == o.shape and torch.equal(o, s.solvevec(m, v, method))
        o = torch.empty(n, 2, N, dtype=TT[dn], device=dev)
        assert s.rmdiv(r, m, method, out=o) is o and torch.equal(o, s.rmdiv(r, m, method))
    o = torch.empty_like(spd)
    assert s.inv(spd, 'chol', out=o) is o and torch.equal(o, s.inv(spd, 'chol'))
    with pytest.raises(ValueError, match='out='):
        s.lmdiv(a, b, out=torch.empty(n, N, 4, dtype=TT[dn], device=dev))
    with pytest.raises(RuntimeError, match='out='):
        s.lmdiv(a.clone().requires_grad_(), b, out=torch.empty_like(b))


# ------------------------------------------------------------------------------------------------ autograd, graphs
@pytest.mark.parametrize('N', [9, 16])
def test_gradcheck(dev, N, monkeypatch):
    s = S()
    g = torch.Generator(device='cpu').manual_seed(5 + N)
    a = (torch.randn(3, N, N, dtype=torch.float64, generator=g) + N * torch.eye(N, dtype=torch.float64)).to(dev)
    b = torch.randn(3, N, 2, dtype=torch.float64, generator=g).to(dev)
    v = torch.randn(3, N, dtype=torch.float64, generator=g).to(dev)
    req = (lambda x: x.clone().requires_grad_())
    families = []
    launch = s._launch
    monkeypatch.setattr(s, '_launch', lambda family, *args: (families.append(family), launch(family, *args))[1])
    a1, b1 = req(a), req(b)
    x = s.lmdiv(a1, b1)
    assert families == [s._ROWSOLVE]
    x.sum().backward()
    assert families == [s._ROWSOLVE, s._ROWSOLVE] and a1.grad.shape == a.shape and b1.grad.shape == b.shape
    a0, b0 = req(a[0]), req(b)                             # one a for every b: its gradient sums to its shape
    s.lmdiv(a0, b0).sum().backward()
    assert a0.grad.shape == (N, N) and b0.grad.shape == b.shape and set(families) == {s._ROWSOLVE}
    ab = req(a[0].expand(3, N, N).contiguous())
    s.lmdiv(ab, b).sum().backward()
    assert torch.allclose(a0.grad, ab.grad.sum(0), rtol=1e-10, atol=1e-12)
    assert torch.autograd.gradcheck(s.lmdiv, (req(a), req(b)))
    assert torch.autograd.gradcheck(s.lmdiv, (req(a[0]), req(b)))
    assert torch.autograd.gradcheck(s.solvevec, (req(a), req(v)))
    assert torch.autograd.gradcheck(lambda y: s.lmdiv(a @ a.mT, y, 'chol'), (req(b),))
    assert set(families) == {s._ROWSOLVE}


def test_graph_capture(dev):
    from nitorch_fastmath_amd import utils
    s = S()
    rng = np.random.default_rng(90)
    mk = (lambda: (t((rng.standard_normal((300, 12, 12)) + 6 * np.eye(12)).astype(np.float32), dev),
                   t(rng.standard_normal((300, 12, 3)).astype(np.float32), dev)))
    a0, b0 = mk()
    step = utils.graphed(lambda a, b: s.lmdiv(a, b), a0, b0)
    for _ in range(2):
        a1, b1 = mk()
        x = step(a1, b1).clone()
        assert torch.equal(x, s.lmdiv(a1, b1))
