"""realtransforms on the GPU.  Every result is compared with the dense float64 matrix of
tests/_realtransforms_ref.py applied on the CPU, per output element within
    |y_k - ref_k| <= (N + 6) eps(dtype) sum_n |M_kn| |x_n| + smallest normal number
(`_realtransforms_ref.bound`: the recursive-summation bound with a few ulps for the coefficient -- derived, not
measured).  Zeros map to exact zeros."""
import numpy as np
import pytest
import torch
import _realtransforms_ref as R

pytestmark = pytest.mark.gpu
TD = {np.float32: torch.float32, np.float64: torch.float64}


@pytest.fixture(scope='module')
def RT():
    from nitorch_fastmath_amd import realtransforms
    return realtransforms


def kinds_types_norms():
    for kind in R.KINDS:
        for type in R.TYPES:
            for norm in R.NORMS:
                yield kind, type, norm


def check(got, M, x, axis, dtype, what, factor=1.0):
    r = R.ratio(got.cpu().numpy(), R.apply(M, x, axis), R.bound(M, x, dtype, axis, factor))
    assert r <= 1, (what, r)
    return r


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_identity_batch_visits_every_coefficient(RT, dev, dtype):
    """unit impulses: every (k, n) of the index arithmetic, every kind, type, norm and transpose setting, with
    the lines along the first axis (lanes along `inner`) and along the last one (tiles through LDS)"""
    from nitorch_fastmath_amd import _lib
    cap = RT.max_len(TD[dtype])
    assert 64 <= cap <= 256
    worst = 0.0
    for N in sorted({1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 64, cap}):
        eye = np.eye(N, dtype=dtype)
        xe = torch.from_numpy(eye).to(dev)
        for kind, type, norm in kinds_types_norms():
            if kind == 'dct' and type == 1 and N == 1:
                continue
            M = R.matrix(kind, type, norm, N)
            for tr in (False, True):
                want = M.T if tr else M
                for axis in (0, 1):
                    got = RT._apply(xe, [axis], R.KINDS.index(kind), type, norm, tr)
                    w = want if axis == 0 else want.T       # lines along axis 1: row n holds column n
                    g = got.cpu().numpy()
                    r = R.ratio(g, w, R.bound(want, eye, dtype, axis=0) if axis == 0 else R.bound(want, eye, dtype, axis=0).T)
                    worst = max(worst, r)
                    assert r <= 1, (kind, type, norm, N, tr, axis, r)
                    assert np.all(g[w == 0] == 0)
    print(f'identity batch, {np.dtype(dtype).name}: worst fraction of the bound {worst:.3f}')


def layouts(N, dev, dtype, rng):
    """(name, tensor on the device, axis)"""
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(dtype)).to(dev)  # noqa: E731
    yield 'last axis, ragged second tile', t(300, N), -1
    yield 'first axis', t(N, 300), 0
    yield 'middle axis, inner 67', t(5, N, 67), 1
    yield 'middle axis, inner 128', t(3, N, 128), 1
    yield 'transposed view', t(300, N).t(), 0
    yield 'step-2 slice', t(40, 2 * N)[:, ::2], 1
    off = t(3 * N * 20 + 1)[1:].view(3, N, 20)
    assert off.data_ptr() % 16 != 0
    yield 'base one element off 16 bytes', off, 1
    off = t(50 * N + 1)[1:].view(50, N)
    yield 'last axis, base off 16 bytes', off, 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('N', [3, 17, 33, 64])
def test_layouts(RT, dev, dtype, N):
    rng = np.random.default_rng(100 + N)
    combos = [('dct', 2, 'backward'), ('dst', 3, 'ortho'), ('dct', 1, 'forward'), ('dst', 1, 'ortho_scipy'),
              ('dct', 3, 'ortho_scipy'), ('dst', 2, 'ortho_scipy')]
    for name, x, axis in layouts(N, dev, dtype, rng):
        xc = x.cpu().numpy()
        before = x.clone()
        for kind, type, norm in combos:
            got = getattr(RT, kind)(x, axis, norm, type)
            assert got.shape == x.shape and got.dtype == x.dtype
            check(got, R.matrix(kind, type, norm, N), xc, axis, dtype, (name, kind, type, norm))
        assert torch.equal(x, before), 'the input is left alone'


def test_nan_stays_in_its_line(RT, dev):
    for shape, axis, line in (((300, 17), 1, (131, slice(None))), ((17, 300), 0, (slice(None), 131)),
                              ((4, 17, 12), 1, (2, slice(None), 8))):
        x = torch.randn(shape, device=dev)
        clean = RT.dst(x, axis, 'ortho', 2)
        x[line][3] = float('nan')
        got = RT.dst(x, axis, 'ortho', 2)
        assert torch.isnan(got[line]).all()
        mask = torch.ones(shape, dtype=torch.bool, device=dev)
        mask[line] = False
        assert torch.equal(got[mask], clean[mask])
    assert torch.equal(RT.dctn(torch.zeros(5, 9, 4, device=dev)), torch.zeros(5, 9, 4, device=dev))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_round_trips(RT, dev, dtype):
    """inverse(forward(x)) == x within twice the bound of the composed matrix |M_inv| |M| (both passes round),
    every type and norm ('ortho_scipy' included: the first-term corrections of DST-II and DST-III cancel)"""
    rng = np.random.default_rng(5)
    for N in (5, 33):
        xc = rng.standard_normal((40, N)).astype(dtype)
        x = torch.from_numpy(xc).to(dev)
        for kind, type, norm in kinds_types_norms():
            back = getattr(RT, 'i' + kind)(getattr(RT, kind)(x, -1, norm, type), -1, norm, type)
            A = np.abs(R.inverse_matrix(kind, type, norm, N)) @ np.abs(R.matrix(kind, type, norm, N))
            b = 2 * (N + 6) * R.eps_of(dtype) * (np.abs(xc).astype(np.float64) @ A.T) + np.finfo(dtype).tiny
            assert R.ratio(back.cpu().numpy(), xc.astype(np.float64), b) <= 1, (kind, type, norm, N)


def test_nd_forms_and_in_place_passes(RT, dev):
    rng = np.random.default_rng(9)
    xc = rng.standard_normal((6, 5, 7))
    x = torch.from_numpy(xc).to(dev)
    for kind, type, norm in kinds_types_norms():
        for dims in ([0, 2], None):
            got = getattr(RT, kind + 'n')(x, dims, norm, type).cpu().numpy()
            want, bnd = xc, np.abs(xc)
            for d in (dims if dims is not None else [0, 1, 2]):
                M = R.matrix(kind, type, norm, xc.shape[d])
                want = R.apply(M, want, d)
                bnd = R.apply(np.abs(M), bnd, d)
            # every pass rounds what the later passes amplify: the bound of the composed |M| with the pass count
            npass = 2 if dims is not None else 3
            b = npass * (7 + 6) * R.eps_of(np.float64) * bnd + np.finfo(np.float64).tiny
            assert R.ratio(got, want, b) <= 1, (kind, type, norm, dims)
    # a pass whose output is its input, straight through the C ABI
    from nitorch_fastmath_amd import _lib
    from nitorch_fastmath_amd._dispatch import call
    for shape, d in (((300, 33), 1), ((33, 300), 0), ((6, 5, 7), 1)):
        y = torch.randn(shape, device=dev)
        want = RT.dct(y, d, 'ortho', 2)
        outer = int(np.prod(shape[:d], dtype=np.int64))
        inner = int(np.prod(shape[d + 1:], dtype=np.int64))
        call(_lib.lib().nfm_rt_transform, dev, 0, 0, 2, 2, 0, shape[d], outer, inner, y.data_ptr(), y.data_ptr())
        assert torch.equal(y, want)


def test_dtype_promotion_and_empty(RT, dev):
    h = torch.randn(20, 9, device=dev).half()
    got = RT.dct(h)
    assert got.dtype == torch.float32 and torch.equal(got, RT.dct(h.float()))
    i = torch.arange(60, device=dev).reshape(4, 15)
    got = RT.dst(i, 0)
    assert got.dtype == torch.float64 and torch.equal(got, RT.dst(i.double(), 0))
    assert RT.dctn(torch.zeros(0, 8, device=dev)).shape == (0, 8)
    with pytest.raises(ValueError):
        RT.dct(torch.ones(4, 1, device=dev), type=1)
    with pytest.raises(ValueError):
        RT.dct(torch.ones(4, 4, device=dev), type=4)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cap_boundary(RT, dev, dtype):
    """N = max_len runs the kernel, N = max_len + 1 the torch composition: both within the bound"""
    cap = RT.max_len(TD[dtype])
    rng = np.random.default_rng(21)
    for N in (cap, cap + 1):
        xc = rng.standard_normal((70, N)).astype(dtype)
        x = torch.from_numpy(xc).to(dev)
        for kind, type, norm in (('dct', 2, 'ortho'), ('dst', 3, 'backward'), ('dct', 1, 'forward'), ('dst', 1, 'ortho')):
            check(getattr(RT, kind)(x, -1, norm, type), R.matrix(kind, type, norm, N), xc, -1, dtype, (kind, type, norm, N))
            check(getattr(RT, kind)(x.t().contiguous(), 0, norm, type), R.matrix(kind, type, norm, N), xc.T, 0, dtype,
                  (kind, type, norm, N, 'first axis'))


def test_autograd_float64(RT, dev):
    x = torch.randn(3, 5, 4, dtype=torch.float64, device=dev, requires_grad=True)
    for kind, type, norm in kinds_types_norms():
        fn = getattr(RT, kind)
        assert torch.autograd.gradcheck(lambda t: fn(t, 1, norm, type), (x,)), (kind, type, norm)
        assert torch.autograd.gradgradcheck(lambda t: fn(t, 1, norm, type), (x,)), (kind, type, norm)
    assert torch.autograd.gradcheck(lambda t: RT.idctn(t, [0, 2], 'ortho', 2), (x,))


def test_backward_is_the_transposed_matrix(RT, dev):
    rng = np.random.default_rng(33)
    gc = rng.standard_normal((300, 33)).astype(np.float32)
    for kind, type, norm in (('dct', 2, 'backward'), ('dst', 3, 'ortho_scipy'), ('dct', 1, 'ortho'), ('dst', 2, 'forward')):
        x = torch.randn(300, 33, device=dev, requires_grad=True)
        y = getattr(RT, kind)(x, -1, norm, type)
        (gx,) = torch.autograd.grad(y, x, torch.from_numpy(gc).to(dev))
        check(gx, R.matrix(kind, type, norm, 33).T, gc, -1, np.float32, (kind, type, norm))


def test_graph_capture(RT, dev):
    x = torch.randn(4, 33, 64, device=dev)
    eager = RT.dctn(x, [1, 2], 'ortho', 2)          # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = RT.dctn(x, [1, 2], 'ortho', 2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.mul_(2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, RT.dctn(x, [1, 2], 'ortho', 2))
