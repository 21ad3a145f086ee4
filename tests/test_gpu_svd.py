"""The Jacobi SVD solves of `sugar` on the GPU: `lmdiv` / `rmdiv` / `solvevec` / `inv` with method 'svd' / 'pinv'
and every non-square system of at most 8 rows and columns run `nfm_svd_solve` -- never torch's SVD --, agree with
the reference's results (tests/golden/svd.npz), meet per-record bounds on graded square and on rectangular
records, cut the singular values where numpy's float64 `pinv` cuts them, keep a singular record's inf / NaN to
that record, read every layout in place, and replay from a HIP graph.

Bounds.  Square: the backward error `solve_eta` of tests/_solver_ref.py per column of every record against
`eta_bound` (2 eta_ref + 4 N eps), the reference being the reference's own composition in torch on the CPU in the
same dtype.  Rectangular: the forward error against numpy's float64 `pinv(a) @ b`, at most
2 err_ref + 4 max(M, N) eps cond_2(A) (tests/_svd_ref.py)."""
import os
import numpy as np
import pytest
import torch
from conftest import GOLDEN
import _solver_ref as R
import _svd_ref as V

pytestmark = pytest.mark.gpu
DNS = ['f32', 'f64']
NS = (1, 65, 209)
TT = V.TT


def S():
    from nitorch_fastmath_amd import sugar
    return sugar


def t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)


def c(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'svd.npz'))


def square_ref(a, b, method):
    """the reference's composition (sugar.py:130-135) in torch on the CPU"""
    a, b = torch.from_numpy(np.array(a)), torch.from_numpy(np.array(b))
    if method == 'svd':
        u, s, v = torch.svd(a)
        return torch.matmul(v, u.transpose(-1, -2).matmul(b) / s[..., None]).numpy()
    return torch.matmul(torch.linalg.pinv(a, rcond=1e-15), b).numpy()


def column_excess(a, got, ref, b, N, dn, what):
    """solve_eta / eta_bound of every column of every record; every record has a verdict"""
    worst = 0.0
    for col in range(b.shape[-1]):
        eta = R.solve_eta(a, got[..., col], b[..., col], dn)
        eref = R.solve_eta(a, ref[..., col], b[..., col], dn)
        ex = eta / R.eta_bound(eref, N, dn)
        assert not np.isnan(ex).any(), what
        w, i = R.worst(ex)
        print(f'{what} col {col}: worst eta / bound = {w:.3g} (record {i}), worst eta / (N eps) = '
              f'{eta.max() / (N * R.EPS[dn]):.3g}, reference {eref.max() / (N * R.EPS[dn]):.3g}')
        assert w <= 1.0, (what, col, f'record {i}: {w:.3g} times its bound')
        worst = max(worst, w)
    return worst


# ------------------------------------------------------------------------------------------------ no torch route
@pytest.mark.parametrize('dn', DNS)
def test_no_torch_route(dev, dn, monkeypatch):
    """with torch's SVD and pseudo-inverse out of reach, everything up to 8 x 8 still answers; order 12 does not"""
    s = S()
    rng = np.random.default_rng(10)
    mk = (lambda *shape: t(rng.standard_normal(shape).astype(V.NP[dn]), dev))
    a, b, v, ar = mk(65, 4, 4) + 4 * torch.eye(4, dtype=TT[dn], device=dev), mk(65, 4, 3), mk(65, 4), mk(65, 2, 4)
    tall, wide, big = mk(65, 8, 3), mk(65, 3, 8), mk(5, 12, 12)

    def gone(*args, **kwargs):
        raise AssertionError('the torch route was taken')
    monkeypatch.setattr(torch, 'svd', gone)
    monkeypatch.setattr(torch.linalg, 'svd', gone)
    monkeypatch.setattr(torch.linalg, 'pinv', gone)
    for method in ('svd', 'pinv'):
        x = s.lmdiv(a, b, method)
        assert x.shape == (65, 4, 3) and torch.isfinite(x).all()
        assert torch.allclose(a @ x, b, atol=1e-3 if dn == 'f32' else 1e-10)
        assert s.inv(a, method).shape == (65, 4, 4) and s.solvevec(a, v, method).shape == (65, 4)
        assert torch.allclose(s.rmdiv(ar, a, method) @ a, ar, atol=1e-3 if dn == 'f32' else 1e-10)
    x = s.lmdiv(tall, mk(65, 8, 2))
    assert x.shape == (65, 3, 2) and torch.isfinite(x).all()
    p = s.inv(wide)
    assert p.shape == (65, 8, 3) and torch.allclose(wide @ p, torch.eye(3, dtype=TT[dn], device=dev).expand(65, 3, 3),
                                                    atol=1e-3 if dn == 'f32' else 1e-10)
    for call in (lambda: s.lmdiv(big, mk(5, 12, 2), 'svd'), lambda: s.inv(big, 'pinv'), lambda: s.lmdiv(big[:, :, :9], mk(5, 12, 2))):
        with pytest.raises(AssertionError, match='torch route'):
            call()


# ------------------------------------------------------------------------------------------------ golden parity
@pytest.mark.parametrize('dn', DNS)
def test_golden_parity(dev, golden, dn):
    s = S()

    def hold(got, ref, truth, M, N, what):
        tr, cond, den = truth
        got = c(got)
        assert got.shape == ref.shape and got.dtype == ref.dtype, what
        err, eref = V.rec_err(got, tr, den), V.rec_err(ref, tr, den)
        ex = err / (2.0 * eref + 4.0 * max(M, N) * V.EPS[dn] * cond)
        print(f'{what} {dn}: worst err / bound = {ex.max():.3g}')
        assert ex.max() <= 1.0, (what, ex.max())

    for M, N in ((2, 1), (1, 4), (8, 3), (3, 8), (7, 5), (5, 7), (8, 7)):
        def G(k):
            return golden[f'{dn}_{M}x{N}_{k}']
        a, b, v, ar = G('a'), G('b'), G('v'), G('ar')
        ad = t(a, dev)
        hold(s.lmdiv(ad, t(b, dev)), G('lmdiv'), V.truth(a, b), M, N, f'lmdiv {M}x{N}')
        hold(s.inv(ad), G('inv'), V.truth(a, None), M, N, f'inv {M}x{N}')
        tv = V.truth(a, v[..., None])
        hold(s.solvevec(ad, t(v, dev)), G('solvevec'), (tv[0][..., 0],) + tv[1:], M, N, f'solvevec {M}x{N}')
        at, art = a.transpose(0, 2, 1), ar.transpose(0, 2, 1)
        tt = V.truth(at, art)                               # X a = ar is a^T X^T = ar^T
        hold(s.rmdiv(t(ar, dev), ad), V.torch_ref(at, art).transpose(0, 2, 1).copy(), (G('rmdiv'),) + tt[1:], M, N, f'rmdiv {M}x{N}')
    rc = {'f32': 1e-6, 'f64': 1e-13}[dn]
    a, b = golden[f'{dn}_rank7_a'], golden[f'{dn}_rank7_b']
    hold(s.lmdiv(t(a, dev), t(b, dev), 'pinv', rcond=rc), golden[f'{dn}_rank7_lmdiv'], V.truth(a, b, rc), 8, 8, 'rank 7 pinv')


# ------------------------------------------------------------------------------------------------ per-record accuracy
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', [1, 3, 8])
def test_square_graded_per_record(dev, dn, N):
    """general_graded, every cond, every record times its own power of two, n = 1, 65, 209, K = 1, 3, both methods:
    eta <= 2 eta_ref + 4 N eps for every column of every record"""
    s = S()
    for cond in R.CONDS[dn]:
        for n in NS:
            k = R.pow2_scales(n, R.KMAX_LINEAR[dn], 900 + N)
            a = R.scaled(R.general_graded(n, N, cond, dn, 200 + N)[0], k)
            for K in (1, 3):
                b = np.random.default_rng(910 + K).standard_normal((n, N, K)).astype(R.NP[dn])
                for method in ('svd', 'pinv'):
                    got = c(s.lmdiv(t(a, dev), t(b, dev), method))
                    ref = square_ref(a, b, method)
                    assert got.shape == (n, N, K) and np.isfinite(ref).all(), (method, cond, n, K)
                    column_excess(a, got, ref, b, N, dn, f'{method} N={N} {dn} cond={cond:g} n={n} K={K}')


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('shape', V.RECT_SHAPES)
def test_rectangular_per_record(dev, dn, shape):
    s = S()
    M, N = shape
    for n in NS:
        a, b = (x[:n] for x in V.rect_case(209, M, N, 3, dn))
        got = c(s.lmdiv(t(a, dev), t(b, dev)))
        assert got.shape == (n, N, 3)
        assert V.rect_excess(got, a, b, dn, what=f'lmdiv n={n}').max() <= 1.0
    pin = c(s.inv(t(a, dev)))
    assert V.rect_excess(pin, a, None, dn, what='inv').max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
def test_pinv_threshold(dev, dn):
    """one singular value at rcond sigma_max 10^(+-1.5): kept or dropped as numpy's float64 pinv does"""
    s = S()
    rc = {'f32': 1e-3, 'f64': 1e-8}[dn]
    for M, N in ((5, 5), (8, 3), (3, 8)):
        a, b = V.threshold_case(65, M, N, dn, rc, 300 + M)
        got = c(s.lmdiv(t(a, dev), t(b, dev), 'pinv', rcond=rc))
        assert V.rect_excess(got, a, b, dn, rc, what='threshold').max() <= 1.0
        if M == N:      # and 'svd' keeps every one of them
            full = c(s.lmdiv(t(a, dev), t(b, dev), 'svd', rcond=rc))
            assert V.rect_excess(full, a, b, dn, 1e-15, what='no threshold').max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('pos', [0, 63, 64, 129])
def test_singular_record_is_alone(dev, dn, pos):
    s = S()
    N, n = 5, 130
    a = R.general_graded(n, N, R.CONDS[dn][0], dn, 205)[0].copy()
    b = np.random.default_rng(82).standard_normal((n, N, 3)).astype(R.NP[dn])
    clean = s.lmdiv(t(a, dev), t(b, dev), 'svd')
    bad = a.copy()
    bad[pos, 2] = 0.0                                   # a zero row: sigma = 0 exactly
    got = s.lmdiv(t(bad, dev), t(b, dev), 'svd')
    assert not torch.isfinite(got[pos]).any()
    rest = torch.arange(n, device=dev) != pos
    assert torch.equal(got[rest], clean[rest]) and torch.isfinite(clean).all()
    gi, ci = s.inv(t(bad, dev), 'svd'), s.inv(t(a, dev), 'svd')
    assert not torch.isfinite(gi[pos]).any() and torch.equal(gi[rest], ci[rest])


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('shape', [(4, 4), (8, 3), (3, 8)])
def test_layouts_read_in_place(dev, dn, shape):
    s = S()
    M, N = shape
    n, K = 200, 3
    a, b = V.rect_case(209, M, N, K, dn)
    a, b = a[:n], b[:n]
    ad, bd = t(a, dev), t(b, dev)
    method = 'pinv'
    base = s.lmdiv(ad, bd, method)
    assert V.rect_excess(c(base), a, b, dn, what='contiguous').max() <= 1.0

    def same(x, what, aa=a, bb=b):
        x = c(x).reshape(-1, N, bb.shape[-1])
        assert V.rect_excess(x, aa, bb, dn, what=what).max() <= 1.0
    at = t(a.transpose(0, 2, 1).copy(), dev).mT
    assert not at.is_contiguous()
    same(s.lmdiv(at, bd, method), 'a.mT')
    # channel-first a, b and result
    cf = (lambda x: x.reshape(8, 25, *x.shape[1:]).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    acf, bcf = cf(ad), cf(bd)
    assert acf.stride(1) == 1 and bcf.stride(1) == 1
    xcf = s.lmdiv(acf, bcf, method)
    assert xcf.shape == (8, 25, N, K)
    if M == N:
        assert xcf.stride() == bcf.stride()                  # the layout of b is handed on
    same(xcf, 'channel-first')
    ocf = cf(torch.empty(n, N, K, dtype=TT[dn], device=dev))
    assert s.lmdiv(acf, bcf, method, out=ocf) is ocf
    same(ocf, 'channel-first out')
    # one a against many b
    x1 = s.lmdiv(ad[7], bd, method)
    assert x1.shape == (n, N, K)
    same(x1, 'one a', np.broadcast_to(a[7], a.shape))
    # out= aliasing b (the shapes agree for square systems)
    if M == N:
        b2 = bd.clone()
        assert s.lmdiv(ad, b2, method, out=b2) is b2 and torch.equal(b2, base)
    # K = cap + 3: column blocks on views of b and of the result, bit for bit the separate calls on the same views
    cap = s.svd_max_cols(TT[dn], M, N)
    bw = np.random.default_rng(52).standard_normal((n, M, cap + 3)).astype(V.NP[dn])
    bwd = t(bw, dev)
    xw = s.lmdiv(ad, bwd, method)
    assert xw.shape == (n, N, cap + 3) and xw.is_contiguous()
    same(xw, 'column blocks', a, bw)
    for c0 in range(0, cap + 3, cap):
        assert torch.equal(xw[..., c0:c0 + cap], s.lmdiv(ad, bwd[..., c0:c0 + cap], method)), c0


def test_graph_capture(dev):
    from nitorch_fastmath_amd import utils
    s = S()
    rng = np.random.default_rng(90)
    mk = (lambda: (t((rng.standard_normal((300, 4, 4)) + 5 * np.eye(4)).astype(np.float32), dev),
                   t(rng.standard_normal((300, 4, 3)).astype(np.float32), dev)))
    a0, b0 = mk()
    step = utils.graphed(lambda a, b: s.lmdiv(a, b, 'pinv'), a0, b0)
    for _ in range(2):
        a1, b1 = mk()
        x = step(a1, b1).clone()
        assert torch.equal(x, s.lmdiv(a1, b1, 'pinv'))
