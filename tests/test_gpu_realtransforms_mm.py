"""realtransforms on axes past the lane kernels' cap: the matrix-core kernel (nfm_rt_transform_mm) through the C
ABI and through the facade's routing.  Every result is compared with the dense float64 matrix of
tests/_realtransforms_ref.py applied on the CPU, per output element within the bound of the lane kernels,
    |y_k - ref_k| <= (N + 6) eps(dtype) sum_n |M_kn| |x_n| + smallest normal number
(`_realtransforms_ref.bound`): an fma chain of N terms in any order satisfies it.  Zeros map to exact zeros.
The shapes are the smallest at which tiling (16 x 16 result tiles, 32 lines a workgroup, k-steps of 4), padding
and the lane maps of the matrix instructions can go wrong."""
import functools
import numpy as np
import pytest
import torch
import _realtransforms_ref as R

pytestmark = pytest.mark.gpu
TD = {np.float32: torch.float32, np.float64: torch.float64}
CODE = {torch.float32: 0, torch.float64: 1}
COMBOS = [('dct', 2, 'backward'), ('dst', 3, 'ortho'), ('dct', 1, 'forward'), ('dst', 1, 'ortho_scipy'),
          ('dct', 3, 'ortho_scipy'), ('dst', 2, 'ortho_scipy')]          # the six of test_layouts
matrix = functools.lru_cache(maxsize=None)(R.matrix)
inverse_matrix = functools.lru_cache(maxsize=None)(R.inverse_matrix)


@pytest.fixture(scope='module')
def RT():
    from nitorch_fastmath_amd import realtransforms
    return realtransforms


def kinds_types_norms():
    for kind in R.KINDS:
        for type in R.TYPES:
            for norm in R.NORMS:
                yield kind, type, norm


def mm(x, axis, kind, type, norm, tr=False, out=None):
    """nfm_rt_transform_mm along `axis` of a contiguous tensor (`out` may be x itself)"""
    from nitorch_fastmath_amd import _lib
    from nitorch_fastmath_amd._dispatch import call
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    axis %= x.dim()
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    call(_lib.lib().nfm_rt_transform_mm, x.device, CODE[x.dtype], R.KINDS.index(kind), type, R.NORMS.index(norm),
         int(tr), x.shape[axis], outer, inner, x.data_ptr(), out.data_ptr())
    return out


def check(got, M, x, axis, dtype, what, factor=1.0):
    r = R.ratio(got.cpu().numpy(), R.apply(M, x, axis), R.bound(M, x, dtype, axis, factor))
    print(f'{what}: {r:.3f} of the bound')
    assert r <= 1, (what, r)
    return r


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_identity_batch_through_the_c_abi(dev, dtype):
    """unit impulses: every (k, n) of the coefficient index and of the operand / result lane maps, lines along
    axis 0 (coefficients are the A operand) and along axis 1 (the data is).  DCT-II / DST-III are not symmetric:
    a result written with rows and columns swapped fails here."""
    worst = 0.0
    for N in (1, 2, 3, 17, 33, 65, 97, 128, 129, 182, 218, 255, 256):
        eye = np.eye(N, dtype=dtype)
        xe = torch.from_numpy(eye).to(dev)
        for kind, type, norm in (kinds_types_norms() if N < 128 else COMBOS):
            if kind == 'dct' and type == 1 and N == 1:
                continue
            M = matrix(kind, type, norm, N)
            for tr in (False, True):
                want = M.T if tr else M
                b = R.bound(want, eye, dtype, axis=0)
                for axis in (0, 1):
                    g = mm(xe, axis, kind, type, norm, tr).cpu().numpy()
                    w, bw = (want, b) if axis == 0 else (want.T, b.T)   # lines along axis 1: row n holds column n
                    r = R.ratio(g, w, bw)
                    worst = max(worst, r)
                    assert r <= 1, (kind, type, norm, N, tr, axis, r)
                    assert np.all(g[w == 0] == 0), (kind, type, norm, N, tr, axis)
    print(f'identity batch, {np.dtype(dtype).name}: worst fraction of the bound {worst:.3f}')


def layouts(N, dev, dtype, rng):
    """(name, tensor on the device, axis)"""
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(dtype)).to(dev)  # noqa: E731
    yield 'last axis, ragged last tile', t(300, N), -1
    yield 'first axis', t(N, 300), 0
    yield 'middle axis, inner 67', t(5, N, 67), 1
    yield 'middle axis, inner 128', t(3, N, 128), 1
    yield 'a single line, last axis', t(1, N), 1
    yield 'a single line, first axis', t(N, 1), 0
    yield 'fewer lines than a tile', t(7, N), 1
    yield 'transposed view', t(300, N).t(), 0
    yield 'step-2 slice', t(40, 2 * N)[:, ::2], 1
    off = t(3 * N * 20 + 1)[1:].view(3, N, 20)
    assert off.data_ptr() % 16 != 0
    yield 'base one element off 16 bytes', off, 1
    off = t(50 * N + 1)[1:].view(50, N)
    assert off.data_ptr() % 16 != 0
    yield 'last axis, base off 16 bytes', off, 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('N', [65, 129, 256])
def test_layouts(RT, dev, dtype, N):
    rng = np.random.default_rng(200 + N)
    for name, x, axis in layouts(N, dev, dtype, rng):
        xc = x.cpu().numpy()
        before = x.clone()
        for kind, type, norm in COMBOS:
            got = getattr(RT, kind)(x, axis, norm, type)
            assert got.shape == x.shape and got.dtype == x.dtype
            check(got, matrix(kind, type, norm, N), xc, axis, dtype, (name, kind, type, norm))
        assert torch.equal(x, before), 'the input is left alone'


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_guards(dev, dtype):
    """x and out in the middle of NaN-filled buffers, a ragged line count: nothing past the ends is read into a
    result or written"""
    N, pad = 65, 1000
    rng = np.random.default_rng(7)
    for shape, axis in (((37, N), 1), ((N, 37), 0), ((3, N, 13), 1)):
        n = int(np.prod(shape))
        xc = rng.standard_normal(shape).astype(dtype)
        xbuf = torch.full((n + 2 * pad,), float('nan'), dtype=TD[dtype], device=dev)
        obuf = torch.full((n + 2 * pad,), float('nan'), dtype=TD[dtype], device=dev)
        x = xbuf[pad:pad + n].view(shape)
        x.copy_(torch.from_numpy(xc))
        out = obuf[pad:pad + n].view(shape)
        for kind, type, norm in COMBOS:
            mm(x, axis, kind, type, norm, out=out)
            check(out, matrix(kind, type, norm, N), xc, axis, dtype, (shape, kind, type, norm))
            assert torch.isnan(obuf[:pad]).all() and torch.isnan(obuf[pad + n:]).all(), 'guards of the output'
            assert torch.isnan(xbuf[:pad]).all() and torch.isnan(xbuf[pad + n:]).all()
            assert torch.equal(x.cpu(), torch.from_numpy(xc))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_nan_stays_in_its_line(dev, dtype):
    for shape, axis, line in (((300, 65), 1, (131, slice(None))), ((65, 300), 0, (slice(None), 131)),
                              ((4, 65, 12), 1, (2, slice(None), 8))):
        x = torch.randn(shape, device=dev, dtype=TD[dtype])
        clean = mm(x, axis, 'dst', 2, 'ortho')
        assert not torch.isnan(clean).any()
        x[line][3] = float('nan')
        got = mm(x, axis, 'dst', 2, 'ortho')
        assert torch.isnan(got[line]).all()
        mask = torch.ones(shape, dtype=torch.bool, device=dev)
        mask[line] = False
        assert torch.equal(got[mask], clean[mask])
    z = torch.zeros(5, 70, 4, device=dev, dtype=TD[dtype])
    assert torch.equal(mm(z, 1, 'dct', 2, 'ortho'), z)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_in_place(dev, dtype):
    """out == x: a workgroup holds every term of its lines before it writes one"""
    for shape, d in (((300, 129), 1), ((129, 300), 0), ((6, 129, 37), 1)):
        y = torch.randn(shape, device=dev, dtype=TD[dtype])
        for kind, type, norm in (('dct', 2, 'ortho'), ('dst', 3, 'backward')):
            want = mm(y, d, kind, type, norm)
            buf = y.clone()
            mm(buf, d, kind, type, norm, out=buf)
            assert torch.equal(buf, want), (shape, kind)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_routing(RT, dev, dtype):
    td = TD[dtype]
    cap, mcap = RT.max_len(td), RT.mm_max_len(td)
    assert mcap in (64, 128, 256) and mcap >= cap
    x = torch.zeros(2, 2, device=dev, dtype=td)
    assert RT._route(x, cap, False) == 'lane'
    assert RT._route(x, mcap + 1, False) == 'torch'
    assert RT._route(x, cap + 1, True) == 'torch' and RT._route(x.cpu(), cap + 1, False) == 'torch'
    if mcap == cap:                       # the measurement turned the route off for this dtype
        assert RT._route(x, cap + 1, False) == 'torch'
        return
    assert RT._route(x, cap + 1, False) == 'mm' and RT._route(x, mcap, False) == 'mm'
    N = cap + 1
    for shape, axis in (((70, N), 1), ((N, 70), 0), ((3, N, 5), 1)):
        y = torch.randn(shape, device=dev, dtype=td)
        for kind, type, norm in COMBOS:
            got = getattr(RT, kind)(y, axis, norm, type)
            assert torch.equal(got, mm(y, axis, kind, type, norm)), 'the facade runs the matrix-core kernel'


def test_nd_forms_mixing_routes(RT, dev):
    """axes of 66 and 130 take the matrix-core kernel, the axis of 5 a lane kernel; the passes after the first
    run in place"""
    rng = np.random.default_rng(9)
    xc = rng.standard_normal((66, 5, 130))
    x = torch.from_numpy(xc).to(dev)
    for kind, type, norm in kinds_types_norms():
        for dims in ([0, 2], None):
            got = getattr(RT, kind + 'n')(x, dims, norm, type).cpu().numpy()
            want, bnd = xc, np.abs(xc)
            for d in (dims if dims is not None else [0, 1, 2]):
                M = matrix(kind, type, norm, xc.shape[d])
                want = R.apply(M, want, d)
                bnd = R.apply(np.abs(M), bnd, d)
            # every pass rounds what the later passes amplify: the bound of the composed |M| with the pass count
            npass = 2 if dims is not None else 3
            b = npass * (130 + 6) * R.eps_of(np.float64) * bnd + np.finfo(np.float64).tiny
            assert R.ratio(got, want, b) <= 1, (kind, type, norm, dims)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_round_trips(RT, dev, dtype):
    """inverse(forward(x)) == x within twice the bound of the composed matrix |M_inv| |M| (both passes round)"""
    rng = np.random.default_rng(5)
    for N in (65, 182):
        xc = rng.standard_normal((40, N)).astype(dtype)
        x = torch.from_numpy(xc).to(dev)
        for kind, type, norm in kinds_types_norms():
            back = getattr(RT, 'i' + kind)(getattr(RT, kind)(x, -1, norm, type), -1, norm, type)
            A = np.abs(inverse_matrix(kind, type, norm, N)) @ np.abs(matrix(kind, type, norm, N))
            b = 2 * (N + 6) * R.eps_of(dtype) * (np.abs(xc).astype(np.float64) @ A.T) + np.finfo(dtype).tiny
            assert R.ratio(back.cpu().numpy(), xc.astype(np.float64), b) <= 1, (kind, type, norm, N)


def test_autograd_float64(RT, dev):
    """the backward pass is the transposed matrix through the same route"""
    rng = np.random.default_rng(33)
    wc = rng.standard_normal((2, 66, 3))
    w = torch.from_numpy(wc).to(dev)
    for kind, type, norm in (('dct', 2, 'ortho'), ('dst', 1, 'ortho')):
        x = torch.randn(2, 66, 3, dtype=torch.float64, device=dev, requires_grad=True)
        loss = (getattr(RT, kind)(x, 1, norm, type) * w).sum()
        (gx,) = torch.autograd.grad(loss, x)
        check(gx, matrix(kind, type, norm, 66).T, wc, 1, np.float64, ('grad', kind, type, norm))


def test_graph_capture(RT, dev):
    x = torch.randn(4, 65, 130, device=dev)
    eager = RT.dctn(x, None, 'ortho', 2)          # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = RT.dctn(x, None, 'ortho', 2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.mul_(2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, RT.dctn(x, None, 'ortho', 2))
