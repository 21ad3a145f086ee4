"""GPU tests of the special module against tests/golden/special.npz: every fixture case in both dtypes under the
fixture's C, the NaN / inf pattern, layouts, the C ABI in place, the torch route above N = 8, gradients, graph
capture and streams.  Bounds and truths: tests/_special_fixture.py."""
import numpy as np
import pytest
import torch
import _special_fixture as F

pytestmark = pytest.mark.gpu
TD = {'f32': torch.float32, 'f64': torch.float64}


@pytest.fixture(scope='module')
def S(dev):
    import nitorch_fastmath_amd as N
    return N.special


@pytest.fixture(scope='module')
def fx():
    return F.Fixture()


def run(S, kind, prm, x):
    if kind in ('besseliP', 'besseliA'):
        return S.besseli(prm['nu'], x, F.MODES[prm['mode']])
    if kind == 'ratio':
        return S.besseli_ratio(prm['nu'], x, prm['N'], prm['K'])
    return S.mvdigamma(x, prm['order'])


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_golden_forward(S, fx, dev, dt):
    worst = {}
    for kind, key, prm in F.cases():
        x = torch.from_numpy(fx.x(kind, prm)).to(dev, TD[dt])
        got = run(S, kind, prm, x)
        assert got.dtype == TD[dt] and got.shape == x.shape
        C = fx.C(kind, dt)
        r = F.ratio(got.cpu().numpy(), fx.z['T_' + key], fx.bound(kind, key, prm, dt), dt)
        worst[kind] = max(worst.get(kind, 0.0), r / C)
        print(f'{key} {dt} forward ratio {r:.4g} C {C:g}')
        assert r <= C, (key, dt, r, C)
    print(dt, 'worst forward ratio / C per kind:', {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_golden_gradients(S, fx, dev, dt):
    for kind, key, prm in F.cases():
        gi, use = fx.grad_points(kind, key, prm, dt)
        x = torch.from_numpy(fx.x(kind, prm)[gi]).to(dev, TD[dt]).requires_grad_()
        y = run(S, kind, prm, x)
        (g,) = torch.autograd.grad(y, x, torch.ones_like(y))
        C = fx.C(kind, dt)
        r = F.ratio(g.cpu().numpy()[use], fx.z['G_' + key][use], fx.grad_bound(key, dt)[use], dt)
        print(f'{key} {dt} gradient ratio {r:.4g} C {C:g}')
        assert r <= C, (key, dt, r, C)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_special_values(S, fx, dev, dt):
    sp = torch.from_numpy(fx.z['special_x']).to(dev, TD[dt])
    for nu in F.NU_P + F.NU_A:
        for m in range(3):
            with np.errstate(over='ignore'):
                want = fx.z[f'special_bi_{F.tag(nu)}_{m}'].astype(F.NP[dt])
            got = S.besseli(nu, sp, F.MODES[m]).cpu().numpy()
            assert F.same_pattern(got, want), (nu, m, got, want)
    for nu in F.NU_R:
        for N, K in F.NK:
            got = S.besseli_ratio(nu, sp, N, K).cpu().numpy()
            assert F.same_pattern(got, fx.z[f'special_br_{F.tag(nu)}_{N}_{K}'].astype(F.NP[dt])), (nu, N, K, got)
    spd = torch.from_numpy(fx.z['special_dg_x']).to(dev, TD[dt])
    for order in F.ORDERS:
        want = fx.z[f'special_dg_{order}']
        got = S.mvdigamma(spd, order).cpu().numpy()
        assert F.same_pattern(got, want.astype(F.NP[dt])), (order, got)
        if order > 1:       # values at order 1 only: a shifted small argument, rounded in the dtype, sits next to a pole
            continue
        assert F.special_close(got, want, order, fx.C('mvdigamma', dt), dt), (order, got, want)
        wg = fx.z[f'special_dg_grad_{order}']
        fin = np.isfinite(wg) & (np.abs(wg) < float(np.finfo(F.NP[dt]).max))
        xs = spd[torch.from_numpy(fin).to(dev)].clone().requires_grad_()
        (g,) = torch.autograd.grad(S.mvdigamma(xs, order).sum(), xs)
        assert F.special_close(g.cpu().numpy(), wg[fin], order, fx.C('mvdigamma', dt), dt), (order, g, wg[fin])
    # the derivative's limits at z = 0 are numbers, not NaN
    for nu, mode, want in ((1.0, None, 0.5), (1.0, 'norm', 0.5), (2.5, None, 0.0), (0.0, None, 0.0), (0.0, 'norm', -1.0),
                           (0.0, 'log', 0.0), (1.0, 'log', np.inf)):
        z = torch.zeros(3, device=dev, dtype=TD[dt], requires_grad=True)
        (g,) = torch.autograd.grad(S.besseli(nu, z, mode).sum(), z)
        assert (g.cpu().numpy() == want).all(), (nu, mode, g)
    x = torch.zeros(3, device=dev, dtype=TD[dt], requires_grad=True)
    (g,) = torch.autograd.grad(S.besseli_ratio(1.5, x).sum(), x)
    assert torch.equal(g.cpu(), torch.full((3,), 0.2, dtype=TD[dt]))


CALLS = [('besseli0', lambda S, x: S.besseli(0, x, 'log')), ('besseli1', lambda S, x: S.besseli(1, x)),
         ('besseli2p5', lambda S, x: S.besseli(2.5, x, 'norm')), ('ratio', lambda S, x: S.besseli_ratio(0.5, x)),
         ('mvdigamma', lambda S, x: S.mvdigamma(x, 3))]


@pytest.mark.parametrize('name,fn', CALLS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_layouts(S, dev, name, fn, dtype):
    g = torch.Generator().manual_seed(5)
    base = (torch.rand(6, 7, 11, generator=g, dtype=torch.float64) * 30 + 1.5).to(dev, dtype)
    want = fn(S, base.reshape(-1).clone()).reshape(base.shape)
    # permuted-dense: no copy, the result has the input's strides
    p = base.permute(2, 0, 1)
    out = fn(S, p)
    assert out.stride() == p.stride() and torch.equal(out, want.permute(2, 0, 1))
    # non-contiguous (gaps): one copy, same values
    assert torch.equal(fn(S, base[:, ::2, 1:]), want[:, ::2, 1:])
    # 0-dim, empty, odd lengths (scalar tail) and a base pointer off the 16-byte grid
    s = fn(S, base[2, 3, 4])
    assert s.dim() == 0 and torch.equal(s, want[2, 3, 4])
    assert fn(S, base[:0]).shape == (0, 7, 11)
    flat, wflat = base.reshape(-1), want.reshape(-1)
    for n in (1, 2, 3, 5, 63, 257, 461):
        for off in (0, 1, 3):
            assert torch.equal(fn(S, flat[off:off + n]), wflat[off:off + n]), (n, off)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_abi_in_place(S, dev, dtype):
    from nitorch_fastmath_amd import _lib
    from nitorch_fastmath_amd._dispatch import dtype_code, stream_ptr
    L = _lib.lib()
    x = (torch.rand(1001, dtype=torch.float64) * 40 + 0.5).to(dev, dtype)
    sp = stream_ptr(dev)
    for want, call in ((S.besseli(0, x, 'log'), lambda b: L.nfm_special_besseli(dtype_code(dtype), 2, 0.0, b.numel(), b.data_ptr(), b.data_ptr(), sp)),
                       (S.besseli(3.5, x, 'norm'), lambda b: L.nfm_special_besseli(dtype_code(dtype), 1, 3.5, b.numel(), b.data_ptr(), b.data_ptr(), sp)),
                       (S.besseli_ratio(1.0, x, 2, 3), lambda b: L.nfm_special_besseli_ratio(dtype_code(dtype), 1.0, 2, 3, b.numel(), b.data_ptr(), b.data_ptr(), sp)),
                       (S.mvdigamma(x, 2), lambda b: L.nfm_special_mvdigamma(dtype_code(dtype), 2, b.numel(), b.data_ptr(), b.data_ptr(), sp))):
        buf = x.clone()
        assert call(buf) == 0
        assert torch.equal(buf, want)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_large_n_takes_the_torch_route(S, fx, dev, dt):
    """N = 9 is above the kernel's registers: the recurrence runs in torch ops.  The same torch arithmetic at N = 8
    is held against the fixture's truth under the kernel's bound, and the gradient of either route is the Riccati
    backward kernel on its saved output."""
    x = torch.from_numpy(fx.z['zP']).to(dev, TD[dt])
    xn = fx.z['zP'].astype(np.float64)
    C = fx.C('ratio', dt)
    for nu in (0.0, 2.5):
        assert torch.equal(S.besseli_ratio(nu, x, 9, 10), S._ratio_torch(nu, x, 9, 10))        # the route
        for N, K in ((8, 20), (4, 10)):
            key = f'br_{F.tag(nu)}_{N}_{K}'
            got = S._ratio_torch(nu, x, N, K).cpu().numpy()
            r = F.ratio(got, fx.z['T_' + key], fx.bound('ratio', key, dict(nu=nu, N=N, K=K), dt), dt)
            print(f'torch route {key} {dt} ratio {r:.4g} C {C:g}')
            assert r <= C, (key, dt, r)
        xr = x.clone().requires_grad_()
        y = S.besseli_ratio(nu, xr, 9, 10)
        (g,) = torch.autograd.grad(y, xr, torch.ones_like(y))
        r64 = y.detach().double().cpu().numpy()
        a, b = r64 * r64, (2 * nu + 1) * r64 / xn
        rg = F.ratio(g.cpu().numpy(), 1 - a - b, F.EPS[dt] * (1 + a + b), dt)
        print(f'torch route nu {nu} {dt} gradient ratio {rg:.4g} C {C:g}')
        assert rg <= C, (nu, dt, rg)
    sp = torch.tensor([0.0, float('inf'), float('nan')], device=dev, dtype=TD[dt])
    assert F.same_pattern(S.besseli_ratio(0.5, sp, 9, 10).cpu().numpy(), np.array([0.0, 1.0, np.nan]))
    x0 = torch.zeros(3, device=dev, dtype=TD[dt], requires_grad=True)
    (g,) = torch.autograd.grad(S.besseli_ratio(1.5, x0, 9, 10).sum(), x0)
    assert torch.equal(g.cpu(), torch.full((3,), 0.2, dtype=TD[dt]))


def test_gradcheck(S, dev):
    z = torch.tensor([0.3, 1.7, 3.2, 5.5, 14.0, 47.0], device=dev, dtype=torch.float64, requires_grad=True)
    for nu in (0.5, 2.0, 15.0):
        for mode in (None, 'norm', 'log'):
            assert torch.autograd.gradcheck(lambda t: S.besseli(nu, t, mode), (z,), eps=1e-6, atol=1e-6, rtol=1e-5)
    for nu in (0.0, 1.5):
        assert torch.autograd.gradcheck(lambda t: S.besseli_ratio(nu, t), (z,), eps=1e-6, atol=1e-7, rtol=1e-5)
    for order in (1, 3):
        assert torch.autograd.gradcheck(lambda t: S.mvdigamma(t, order), (z,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_non_contiguous_gradient(S, dev):
    base = (torch.rand(5, 8, dtype=torch.float64) * 10 + 0.5).to(dev)
    x = base.t().clone().t().requires_grad_()       # dense, transposed strides
    y = S.besseli(0.5, x, 'log')
    (g,) = torch.autograd.grad(y, x, torch.ones(5, 8, device=dev, dtype=torch.float64))
    xc = base.clone().requires_grad_()
    (gc,) = torch.autograd.grad(S.besseli(0.5, xc, 'log').sum(), xc)
    assert torch.equal(g, gc)


@pytest.mark.parametrize('name,fn', CALLS)
def test_graph_capture_replays_to_the_same_bits(S, dev, name, fn):
    from nitorch_fastmath_amd import utils
    x = (torch.rand(4099, dtype=torch.float64) * 60 + 0.01).float().to(dev)
    eager = fn(S, x)
    graphed = utils.graphed(lambda t: fn(S, t), x)
    assert torch.equal(graphed(x), eager)
    x2 = (torch.rand(4099, dtype=torch.float64) * 5).float().to(dev)
    assert torch.equal(graphed(x2), fn(S, x2))


def test_non_default_stream(S, dev):
    x = (torch.rand(1 << 16, dtype=torch.float64) * 60 + 0.01).float().to(dev)
    want = [fn(S, x) for _, fn in CALLS]
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        got = [fn(S, x) for _, fn in CALLS]
    st.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
