"""The structure kernels of the compact-symmetric family -- sym_to_full, sym_outer, sym_matmul and the
cotangent kernel nfm_sym_outer2 -- at every order, both dtypes, batches with a ragged last wave / tile, and the
operand layouts the launcher treats differently.  Their input and output records differ in size (K -> M x M,
M -> K, K D + K (K + 1) / 2 -> D (D + 1) / 2).  References and derived bounds: tests/_dense_ref.py (the CPU
oracle passes the same bounds on the same inputs in test_structure_host.py)."""
import functools
import numpy as np
import pytest
import torch
from conftest import TOL, relerr
import _dense_ref as R

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}
LAYOUT_MS = (2, 3, 4, 6, 8, 9, 12, 16)
B, X, Y = 3, 17, 9


def S():
    import nitorch_fastmath_amd as N_
    return N_.sym


def t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)          # (a copy: the cached inputs are read-only)


def same(got, ref):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), relerr(got, ref)


@functools.lru_cache(maxsize=None)
def inputs(n, M, dn):
    mat, vec = R.spd_np(n, M, R.NP[dn], 1000 * M + n)
    mat.setflags(write=False)
    vec.setflags(write=False)
    return mat, vec


# ---- layouts of an (n, C) operand, n = B * X * Y: each returns a view with the same values ---------------
def channel_first(x, comp=1):
    """(B, X, Y, *C) stored (B, *C, X, Y), viewed channel-last: no copy, two batch levels"""
    x4 = x.reshape((B, X, Y) + tuple(x.shape[1:]))
    fwd = (0,) + tuple(range(3, 3 + comp)) + (1, 2)
    back = (0, 1 + comp, 2 + comp) + tuple(range(1, 1 + comp))
    return x4.permute(fwd).contiguous().permute(back)


def soa(x):
    """pure SoA: (C, n).T (component dims flattened for the transposition, then restored)"""
    perm = tuple(range(1, x.dim())) + (0,)
    inv = (x.dim() - 1,) + tuple(range(x.dim() - 1))
    return x.permute(perm).contiguous().permute(inv)


def padded(x, pad=3):
    """records padded to C + 3 (the padding is NaN: reading it would show)"""
    C = x[0].numel()
    buf = torch.full((x.shape[0], C + pad), float('nan'), dtype=x.dtype, device=x.device)
    buf[:, :C] = x.reshape(x.shape[0], C)
    return buf[:, :C].unflatten(-1, tuple(x.shape[1:]))


def every_second(x):
    buf = torch.full((2 * x.shape[0],) + tuple(x.shape[1:]), float('nan'), dtype=x.dtype, device=x.device)
    buf[::2] = x
    return buf[::2]


# =========================================================================== sym_to_full / sym_outer
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', R.ORDERS)
def test_to_full_and_outer_sizes(dev, oracle, dn, M):
    """every order at batches around the wave, the 256-lane and the 512-lane tile: bit-identical"""
    for n in R.NS:
        mat, vec = inputs(n, M, dn)
        same(S().sym_to_full(t(mat, dev)), oracle.sym_to_full(mat))
        same(S().sym_outer(t(vec, dev)), oracle.sym_outer(vec))
        if dn == 'f32':
            r = S().sym_outer(t(vec, dev), dtype=torch.float64)
            assert r.dtype == torch.float64
            same(r, oracle.sym_outer(vec.astype(np.float64)))
            same(S().sym_to_full(t(mat, dev), dtype=torch.float64), oracle.sym_to_full(mat.astype(np.float64)))


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', LAYOUT_MS)
def test_to_full_and_outer_layouts(dev, oracle, dn, M):
    n, K = B * X * Y, M * (M + 1) // 2
    mat, vec = inputs(n, M, dn)
    ref_f, ref_o = oracle.sym_to_full(mat), oracle.sym_outer(vec)
    md, vd = t(mat, dev), t(vec, dev)
    to_full, outer = S().sym_to_full, S().sym_outer
    # channel-first input, two batch levels
    same(to_full(channel_first(md)), ref_f.reshape(B, X, Y, M, M))
    same(outer(channel_first(vd)), ref_o.reshape(B, X, Y, K))
    # pure SoA, every second record, padded records
    for view in (soa, every_second, padded):
        same(to_full(view(md)), ref_f)
        same(outer(view(vd)), ref_o)
    # slices that start at an odd record
    for i0 in (1, 2, 3):
        same(to_full(md[i0:]), ref_f[i0:])
        same(outer(vd[i0:]), ref_o[i0:])
        same(to_full(md[i0:n - 1]), ref_f[i0:n - 1])
    # out= into a padded buffer: the padding is left alone
    buf = torch.full((n, M, M + 1), 7.0, dtype=md.dtype, device=dev)
    r = to_full(md, out=buf[..., :M])
    assert r.data_ptr() == buf.data_ptr()
    same(buf[..., :M], ref_f)
    assert bool((buf[..., M] == 7).all())
    buf = torch.full((n, K + 3), 7.0, dtype=md.dtype, device=dev)
    r = outer(vd, out=buf[:, :K])
    assert r.data_ptr() == buf.data_ptr()
    same(buf[:, :K], ref_o)
    assert bool((buf[:, K:] == 7).all())
    buf = torch.full((n + 5, K), 7.0, dtype=md.dtype, device=dev)          # an odd-offset window of records
    outer(vd[3:], out=buf[3:n])
    same(buf[3:n], ref_o[3:])
    assert bool((buf[:3] == 7).all()) and bool((buf[n:] == 7).all())
    # out= into channel-first storage
    out_cf = torch.empty(B, M, M, X, Y, dtype=md.dtype, device=dev).permute(0, 3, 4, 1, 2)
    to_full(channel_first(md), out=out_cf)
    same(out_cf, ref_f.reshape(B, X, Y, M, M))
    out_cf = torch.empty(B, K, X, Y, dtype=md.dtype, device=dev).movedim(1, -1)
    outer(channel_first(vd), out=out_cf)
    same(out_cf, ref_o.reshape(B, X, Y, K))
    outer(vd.reshape(B, X, Y, M), out=out_cf.zero_())                       # AoS in, channel-first out
    same(out_cf, ref_o.reshape(B, X, Y, K))


# =========================================================================== sym_matmul
def check_matmul(got, j, h, ref, dn, k, d):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if k <= 4 and d <= 4:
        assert np.array_equal(got, ref), (k, d, relerr(got, ref))
        return 0.0
    ex = R.matmul_excess(got, j, h, dn)
    assert ex <= 1.0, (k, d, ex)
    assert relerr(got, ref) <= TOL[dn], (k, d, relerr(got, ref))
    return ex


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('diag', [False, True], ids=['sym', 'diag'])
@pytest.mark.parametrize('n', [65, 1573])
@pytest.mark.parametrize('k', R.KD)
def test_matmul_grid(dev, oracle, dn, diag, n, k):
    """every (k, d): bit-identical to the oracle up to 4 x 4, the derived (T + 4) eps S bound against float64
    numpy (and TOL against the oracle) for the big-order kernel"""
    worst = 0.0
    for d in R.KD:
        j, h = R.matmul_inputs(n, k, d, dn, diag)
        got = S().sym_matmul(t(j, dev), t(h, dev))
        worst = max(worst, check_matmul(got, j, h, oracle.sym_matmul(j, h), dn, k, d))
    print(f'k={k} {dn} n={n}: worst |got - truth| / bound = {worst:.3f}')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('kd', [(2, 2), (3, 3), (3, 2), (4, 4), (5, 3), (3, 6), (9, 9), (16, 2), (2, 16)])
def test_matmul_broadcast_and_dtype(dev, oracle, dn, kd):
    k, d = kd
    n = 257
    for diag in (False, True):
        j, h = R.matmul_inputs(n, k, d, dn, diag)
        jd, hd = t(j, dev), t(h, dev)
        # one hessian (1, Kh) against n jacobians, one jacobian against n hessians
        hb = np.ascontiguousarray(np.broadcast_to(h[:1], h.shape))
        check_matmul(S().sym_matmul(jd, hd[:1]), j, hb, oracle.sym_matmul(j, hb), dn, k, d)
        jb = np.ascontiguousarray(np.broadcast_to(j[:1], j.shape))
        check_matmul(S().sym_matmul(jd[:1], hd), jb, h, oracle.sym_matmul(jb, h), dn, k, d)
        check_matmul(S().sym_matmul(jd[0], hd), jb, h, oracle.sym_matmul(jb, h), dn, k, d)
        if dn == 'f32':
            r = S().sym_matmul(jd, hd, dtype=torch.float64)
            j64, h64 = j.astype(np.float64), h.astype(np.float64)
            check_matmul(r, j64, h64, oracle.sym_matmul(j64, h64), 'f64', k, d)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('kd', [(2, 2), (3, 3), (4, 4), (2, 3), (4, 3), (6, 6), (8, 3), (3, 8), (9, 9), (12, 4),
                                (16, 16)])
def test_matmul_layouts(dev, oracle, dn, kd):
    """the same results from channel-first, SoA, strided, padded and odd-offset operands, a transposed
    jacobian, and into padded / channel-first out= buffers"""
    k, d = kd
    n, Kd = B * X * Y, d * (d + 1) // 2
    mm = S().sym_matmul
    for diag in (False, True):
        j, h = R.matmul_inputs(n, k, d, dn, diag)
        ref = oracle.sym_matmul(j, h)
        jd, hd = t(j, dev), t(h, dev)

        def ok(got, sl=slice(None)):
            check_matmul(got.reshape(-1, Kd), j[sl], h[sl], ref[sl], dn, k, d)
        ok(mm(channel_first(jd, 2), channel_first(hd)))
        ok(mm(channel_first(jd, 2), hd.reshape(B, X, Y, -1)))               # mixed layouts
        ok(mm(soa(jd), soa(hd)))
        ok(mm(jd.permute(1, 2, 0).contiguous().permute(2, 0, 1), hd.t().contiguous().t()))
        ok(mm(every_second(jd), every_second(hd)))
        ok(mm(padded(jd), padded(hd)))
        ok(mm(jd.mT.contiguous().mT, hd))                                   # j stored transposed
        for i0 in (1, 2, 3):
            ok(mm(jd[i0:], hd[i0:]), slice(i0, None))
        buf = torch.full((n, Kd + 3), 7.0, dtype=jd.dtype, device=dev)
        r = mm(jd, hd, out=buf[:, :Kd])
        assert r.data_ptr() == buf.data_ptr()
        ok(buf[:, :Kd])
        assert bool((buf[:, Kd:] == 7).all())
        out_cf = torch.empty(B, Kd, X, Y, dtype=jd.dtype, device=dev).movedim(1, -1)
        mm(channel_first(jd, 2), channel_first(hd), out=out_cf)
        ok(out_cf)


# =========================================================================== nfm_sym_outer2
def outer2(x, y, neg=False):
    from nitorch_fastmath_amd import _autograd
    return _autograd.sym_outer2(x, y, neg)


def check_outer2(pos, neg, x, y, dn):
    """`pos` within 2 eps (|x_i y_j| + |x_j y_i|) of the float64 formula; `neg` its exact negation"""
    assert pos.dtype == DT[dn] and pos.shape == tuple(np.broadcast_shapes(x.shape[:-1], y.shape[:-1])) + \
        (x.shape[-1] * (x.shape[-1] + 1) // 2,)
    xb, yb = np.broadcast_arrays(x, y)
    ex = R.outer2_excess(pos.cpu().numpy(), xb, yb, dn)
    assert ex <= 1.0, ex
    assert torch.equal(neg, -pos)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', R.ORDERS)
def test_outer2_sizes(dev, dn, M):
    """Outer2Op (M <= 8) and the big-order kernel (M > 8), float32 included"""
    for n in R.NS:
        x, y = R.outer2_inputs(n, M, dn)
        xd, yd = t(x, dev), t(y, dev)
        check_outer2(outer2(xd, yd), outer2(xd, yd, True), x, y, dn)
        # a (1, M) operand against n records, on either side
        check_outer2(outer2(xd[:1], yd), outer2(xd[:1], yd, True), x[:1], y, dn)
        check_outer2(outer2(xd, yd[:1]), outer2(xd, yd[:1], True), x, y[:1], dn)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', [3, 8, 9, 16])
def test_outer2_layouts(dev, dn, M):
    """every layout within the same derived bound (the kernel variants may contract x_i y_j + x_j y_i into a
    fused multiply-add differently, so they are not compared bit for bit with each other), `neg` exact in each"""
    n = B * X * Y
    x, y = R.outer2_inputs(n, M, dn)
    xd, yd = t(x, dev), t(y, dev)
    K = M * (M + 1) // 2

    def ok(xv, yv, sl=slice(None)):
        pos, neg = outer2(xv, yv), outer2(xv, yv, True)
        check_outer2(pos.reshape(-1, K), neg.reshape(-1, K), x[sl], y[sl], dn)
    ok(xd, yd)
    ok(channel_first(xd), channel_first(yd))
    ok(channel_first(xd), yd.reshape(B, X, Y, M))                           # mixed layouts
    ok(soa(xd), soa(yd))
    ok(xd, soa(yd))
    ok(every_second(xd), every_second(yd))
    ok(padded(xd), padded(yd))
    for i0 in (1, 2, 3):
        ok(xd[i0:], yd[i0:], slice(i0, None))
    # an expanded stride-0 operand (the cotangent of `.sum().backward()`)
    one = torch.ones((), dtype=xd.dtype, device=dev).expand(n, M)
    check_outer2(outer2(one, yd), outer2(one, yd, True), np.ones_like(x), y, dn)
