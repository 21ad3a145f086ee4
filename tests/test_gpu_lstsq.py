"""The tall least-squares solves of `sugar` on the GPU: `lmdiv` / `solvevec` / `rmdiv` of a system with more than 8
rows (up to 4096) and at most 8 columns run `nfm_lstsq_solve` -- never torch's SVD or pseudo-inverse --, meet the
per-record bound of tests/_lstsq_ref.py (2 err_ref + 4 N eps cond_2 against numpy's float64 `pinv(a, rcond) @ b`)
on graded records, over the whole exponent range, at the rcond cut and on rank-deficient records, agree with the
reference's results (tests/golden/lstsq.npz), read every layout in place with the bits of the contiguous call, run
on a side stream and replay from a HIP graph."""
import os
import numpy as np
import pytest
import torch
from conftest import GOLDEN
import _solver_ref as R
import _svd_ref as V
import _lstsq_ref as Q

pytestmark = pytest.mark.gpu
DNS = ['f32', 'f64']
NS = (1, 65, 209)
TT = Q.TT


def S():
    from nitorch_fastmath_amd import sugar
    return sugar


def t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)


def c(x):
    return x.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ no torch route
@pytest.mark.parametrize('dn', DNS)
def test_no_torch_route(dev, dn, monkeypatch):
    """with torch's SVD and pseudo-inverse out of reach, tall systems of at most 8 columns still answer; 12 x 9 and
    a call that needs a gradient do not"""
    s = S()
    rng = np.random.default_rng(11)
    mk = (lambda *shape: t(rng.standard_normal(shape).astype(Q.NP[dn]), dev))
    a, b = mk(65, 33, 6), mk(65, 33, 2)
    a3, v = mk(5, 12, 3), mk(5, 12)
    # X B = A with B 6 x 40: X is 2 x 6 and A 2 x 40 (the system of lmdiv is B^T, 40 x 6, a transposed view)
    ar, br = mk(7, 2, 40), mk(7, 6, 40)
    wide9, g = mk(5, 12, 9), mk(5, 33, 6).requires_grad_()

    def gone(*args, **kwargs):
        raise AssertionError('the torch route was taken')
    monkeypatch.setattr(torch, 'svd', gone)
    monkeypatch.setattr(torch.linalg, 'svd', gone)
    monkeypatch.setattr(torch.linalg, 'pinv', gone)
    x = s.lmdiv(a, b)
    assert x.shape == (65, 6, 2) and x.dtype == TT[dn] and torch.isfinite(x).all()
    assert torch.equal(x, s.lmdiv(a, b, 'svd')) and torch.equal(x, s.lmdiv(a, b, 'pinv'))
    # the normal equations hold: A^T (A x - b) = 0
    tol = 1e-3 if dn == 'f32' else 1e-10
    assert (a.mT @ (a @ x - b)).abs().max() <= tol * 33
    xv = s.solvevec(a3, v)
    assert xv.shape == (5, 3) and torch.isfinite(xv).all()
    xr = s.rmdiv(ar, br)
    assert xr.shape == (7, 2, 6) and torch.isfinite(xr).all()
    assert ((xr @ br - ar) @ br.mT).abs().max() <= tol * 40
    for call in (lambda: s.lmdiv(wide9, mk(5, 12, 2)), lambda: s.lmdiv(g, mk(5, 33, 2)),
                 lambda: s.lmdiv(a[:5], mk(5, 33, 2).requires_grad_())):
        with pytest.raises(AssertionError, match='torch route'):
            call()


# ------------------------------------------------------------------------------------------------ per-record accuracy
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('shape', Q.SHAPES)
def test_per_record(dev, dn, shape):
    s = S()
    M, N, K = shape
    K = s.lstsq_max_cols(TT[dn], N) if K is None else K
    for n in NS:
        a, b = (x[:n] for x in Q.tall_case(209, M, N, K, dn, 4000 + 10 * M + N))
        got = c(s.lmdiv(t(a, dev), t(b, dev)))
        assert got.shape == (n, N, K) and got.dtype == Q.NP[dn]
        assert Q.excess(got, a, b, dn, what=f'lmdiv n={n}').max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
def test_whole_exponent_range(dev, dn):
    s = S()
    kmax = {'f32': 90, 'f64': 900}[dn]
    k = R.pow2_scales(209, kmax, 77)
    a, b = Q.tall_case(209, 33, 6, 1, dn, 4100, exps=tuple(int(v) for v in k))
    got = c(s.lmdiv(t(a, dev), t(b, dev)))
    assert np.isfinite(got).all()
    assert Q.excess(got, a, b, dn, what=f'2^+-{kmax}').max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
def test_cut(dev, dn):
    """the rcond cut at 10^(+-1.5) of the threshold, and records of rank exactly 5 (with R in float32 one float32
    record of these 65 kept a sixth singular value of rounding size at rcond = 1e-6: R is held in double)"""
    s = S()
    rc = {'f32': 1e-4, 'f64': 1e-10}[dn]
    a, b = V.threshold_case(66, 33, 6, dn, rc, 4200)
    got = c(s.lmdiv(t(a, dev), t(b, dev), rcond=rc))
    assert Q.excess(got, a, b, dn, rc, what='threshold').max() <= 1.0
    rc = {'f32': 1e-6, 'f64': 1e-13}[dn]
    a, b = Q.rank5_case(65, dn, 4300)
    got = c(s.lmdiv(t(a, dev), t(b, dev), rcond=rc))
    assert Q.excess(got, a, b, dn, rc, what='rank 5').max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
def test_golden_parity(dev, dn):
    s = S()
    g = np.load(os.path.join(GOLDEN, 'lstsq.npz'))
    for M, N in ((12, 3), (33, 6), (64, 8)):
        a, b, ref = (g[f'{dn}_{M}x{N}_{k}'] for k in ('a', 'b', 'lmdiv'))
        got = c(s.lmdiv(t(a, dev), t(b, dev)))
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert Q.excess(got, a, b, dn, what='golden', ref=ref).max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
def test_nan_record_is_alone(dev, dn):
    s = S()
    a, b = Q.tall_case(209, 33, 6, 2, dn, 4500)
    clean = s.lmdiv(t(a, dev), t(b, dev))
    for pos in (0, 63, 64, 208):
        bad = a.copy()
        bad[pos, 17, 3] = np.nan
        got = s.lmdiv(t(bad, dev), t(b, dev))
        rest = torch.arange(209, device=dev) != pos
        assert torch.isnan(got[pos]).all() and torch.equal(got[rest], clean[rest])
    zero = a.copy()
    zero[5] = 0
    assert (s.lmdiv(t(zero, dev), t(b, dev))[5] == 0).all()


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('shape', [(33, 6), (17, 3), (12, 8)])
def test_layouts_read_in_place(dev, dn, shape):
    """every layout of the same values gives the bits of the contiguous call"""
    s = S()
    M, N = shape
    n, K = 209, 2
    a, b = Q.tall_case(209, M, N, K, dn, 4600 + M)
    ad, bd = t(a, dev), t(b, dev)
    base = s.lmdiv(ad, bd)
    assert base.shape == (n, N, K) and base.is_contiguous()
    assert Q.excess(c(base), a, b, dn, what='contiguous').max() <= 1.0
    # channel-first a and b: movedim views of (M, N, n) storage; the result takes the layout of no operand
    acf = ad.permute(1, 2, 0).contiguous().movedim(-1, 0)
    bcf = bd.permute(1, 2, 0).contiguous().movedim(-1, 0)
    assert acf.stride() == (1, N * n, n) and bcf.stride() == (1, K * n, n)
    xcf = s.lmdiv(acf, bcf)
    print(f'channel-first against contiguous: max |difference| / max |x| = {float((xcf - base).abs().max() / base.abs().max()):.3g}')
    assert torch.equal(xcf, base)
    assert torch.equal(s.lmdiv(acf, bd), base) and torch.equal(s.lmdiv(ad, bcf), base)
    # a.mT of an (N x M) tensor
    at = ad.mT.contiguous().mT
    assert not at.is_contiguous() and at.stride() == (M * N, 1, M)
    assert torch.equal(s.lmdiv(at, bd), base)
    # one system against 209 right-hand sides, and the converse
    x1 = s.lmdiv(ad[7], bd)
    assert x1.shape == (n, N, K) and torch.equal(x1, s.lmdiv(ad[7].expand(n, M, N).contiguous(), bd))
    x2 = s.lmdiv(ad, bd[7])
    assert x2.shape == (n, N, K) and torch.equal(x2, s.lmdiv(ad, bd[7].expand(n, M, K).contiguous()))
    # padded records: slices of a larger last dim
    ap = torch.zeros(n, M, N + 3, dtype=TT[dn], device=dev)
    bp = torch.zeros(n, M, K + 1, dtype=TT[dn], device=dev)
    ap[..., :N], bp[..., 1:] = ad, bd
    assert torch.equal(s.lmdiv(ap[..., :N], bp[..., 1:]), base)
    # two batch levels that do not collapse
    a2 = torch.zeros(11, 21, M, N, dtype=TT[dn], device=dev)[:, :19]
    a2.copy_(ad.reshape(11, 19, M, N))
    assert torch.equal(s.lmdiv(a2, bd.reshape(11, 19, M, K)).reshape(n, N, K), base)
    # out= given, contiguous and channel-first
    out = torch.empty(n, N, K, dtype=TT[dn], device=dev)
    assert s.lmdiv(ad, bd, out=out) is out and torch.equal(out, base)
    ocf = torch.empty(N, K, n, dtype=TT[dn], device=dev).movedim(-1, 0)
    assert s.lmdiv(acf, bcf, out=ocf) is ocf and torch.equal(ocf, base)
    with pytest.raises(ValueError):
        s.lmdiv(ad, bd, out=torch.empty(n, N, K + 1, dtype=TT[dn], device=dev))
    # K = cap + 1 and 2 cap + 1: column blocks on views of b and of the result
    cap = s.lstsq_max_cols(TT[dn], N)
    for kw in (cap + 1, 2 * cap + 1):
        bw = t(np.random.default_rng(52).standard_normal((n, M, kw)).astype(Q.NP[dn]), dev)
        xw = s.lmdiv(ad, bw)
        assert xw.shape == (n, N, kw) and xw.is_contiguous()
        for c0 in range(0, kw, cap):
            assert torch.equal(xw[..., c0:c0 + cap], s.lmdiv(ad, bw[..., c0:c0 + cap].contiguous())), (kw, c0)
    # n = 0
    x0 = s.lmdiv(ad[:0], bd[:0])
    assert x0.shape == (0, N, K)
    # solvevec and rmdiv are the same call on views
    assert torch.equal(s.solvevec(ad, bd[..., 0]), s.lmdiv(ad, bd[..., :1])[..., 0])
    assert torch.equal(s.rmdiv(bd.mT, ad.mT), base.mT)


# ------------------------------------------------------------------------------------------------ streams, graphs, ABI
def test_side_stream(dev):
    s = S()
    a, b = (t(x, dev) for x in Q.tall_case(209, 33, 6, 2, 'f32', 4700))
    base = s.lmdiv(a, b)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        x = s.lmdiv(a, b)
    st.synchronize()
    assert torch.equal(x, base)


def test_graph_capture(dev):
    from nitorch_fastmath_amd import utils
    s = S()
    rng = np.random.default_rng(91)
    mk = (lambda: (t(rng.standard_normal((65, 33, 6)).astype(np.float32), dev),
                   t(rng.standard_normal((65, 33, 2)).astype(np.float32), dev)))
    a0, b0 = mk()
    step = utils.graphed(lambda a, b: s.lmdiv(a, b), a0, b0)
    for _ in range(2):
        a1, b1 = mk()
        x = step(a1, b1).clone()
        assert torch.equal(x, s.lmdiv(a1, b1))


@pytest.mark.parametrize('dn', DNS)
def test_c_abi_direct(dev, dn):
    """pointers from torch tensors, two batch levels: (n_outer, n_inner) = (3, 70) with padded outer slabs"""
    from nitorch_fastmath_amd import _lib
    s = S()
    M, N, K = 17, 3, 2
    a, b = (t(x, dev) for x in Q.tall_case(209, M, N, K, dn, 4617)[:2])
    base = s.lmdiv(a, b)
    A = torch.zeros(3, 75, M, N, dtype=TT[dn], device=dev)
    B = torch.zeros(3, 75, M, K, dtype=TT[dn], device=dev)
    X = torch.full((3, 75, N, K), 7.0, dtype=TT[dn], device=dev)
    for o in range(3):
        A[o, :70 if o < 2 else 69] = a[70 * o:70 * o + 70]
        B[o, :70 if o < 2 else 69] = b[70 * o:70 * o + 70]
    torch.cuda.synchronize()
    rc = _lib.lib().nfm_lstsq_solve(Q.CODE[dn], M, N, K, 1e-15, 3, 70,
                                    A.data_ptr(), 75 * M * N, M * N, N, 1, B.data_ptr(), 75 * M * K, M * K, K, 1,
                                    X.data_ptr(), 75 * N * K, N * K, K, 1, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = torch.cat([X[0, :70], X[1, :70], X[2, :69]])
    assert torch.equal(got, base) and (X[:, 70:] == 7.0).all() and (X[2, 69] == 0).all()
    # one level, contiguous: the LDS-staged kernel
    X1 = torch.empty(209, N, K, dtype=TT[dn], device=dev)
    rc = _lib.lib().nfm_lstsq_solve(Q.CODE[dn], M, N, K, 1e-15, 1, 209, a.data_ptr(), 0, M * N, N, 1,
                                    b.data_ptr(), 0, M * K, K, 1, X1.data_ptr(), 0, N * K, K, 1, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(X1, base)
