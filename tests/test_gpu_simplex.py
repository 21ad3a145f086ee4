"""GPU tests of nitorch_fastmath_amd.simplex against tests/golden/simplex.npz (the real reference's
outputs; bounds and C in tests/_simplex_fixture.py and profiles/simplex_accuracy.md)."""
import itertools
import numpy as np
import pytest
import torch
import _simplex_fixture as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TD = {'f32': torch.float32, 'f64': torch.float64}


@pytest.fixture(scope='module')
def fx():
    return F.Fixture()


@pytest.fixture(scope='module')
def S():
    import nitorch_fastmath_amd as N
    return N.simplex


def run(S, fn, x, imp, idx, dim=1):
    if fn == 'logsumexp':
        return S.logsumexp(x, dim, True, imp[0])
    return getattr(S, fn)(x, dim, imp, idx)


def same_bits(a, o):
    """equal bit for bit (any NaN equals any NaN)"""
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    a, o = a.contiguous(), o.contiguous()
    if a.shape != o.shape or not torch.equal(a.isnan(), o.isnan()):
        return False
    return torch.equal(torch.nan_to_num(a).view(it), torch.nan_to_num(o).view(it))


def grad_bound(fn, x64, go64, imp, idx, dt, C):
    """bound of a float `dt` grad_input against the float64 one: the softmax bound C eps (K' + max |x - m|) T + tiny
    with T, per element, the magnitudes that meet before they cancel:
      softmax      p_k (|g_k| + sum |g p|)      log_softmax  |g_k| + p_k sum |g|      logsumexp  p_k |g|
    The class an explicit input's softmax dropped is rebuilt by the backward pass as 1 - sum(p) from the one saved
    tensor: an absolute eps K' on p there, i.e. eps K' sum |g p| on its gradient, which T gets on top."""
    K = x64.shape[1]
    kp = K + imp[0]
    j = idx % kp
    zero = torch.zeros_like(x64[:, :1])
    z = torch.cat([x64[:, :j], zero, x64[:, j:]], 1) if imp[0] else x64
    p = torch.softmax(z, 1)
    if fn == 'logsumexp':
        t = p * go64.abs()
    else:
        g = torch.cat([go64[:, :j], zero, go64[:, j:]], 1) if imp[1] else go64
        if fn == 'softmax':
            dot = (g * p).abs().sum(1, keepdim=True)
            t = p * (g.abs() + dot)
            if imp[1] and not imp[0]:
                t[:, j] += kp * dot[:, 0]
        else:
            t = g.abs() + p * g.abs().sum(1, keepdim=True)
    if imp[0]:
        t = torch.cat([t[:, :j], t[:, j + 1:]], 1)
    spread = (z - z.amax(1, keepdim=True)).abs().amax(1, keepdim=True)
    return C * F.EPS[dt] * (kp + spread) * t + F.TINY[dt]


def test_golden_accuracy_and_nan_pattern(S, fx):
    """every fixture case, per element, within C x bound of the float64 truth; NaN / inf where the reference has them"""
    worst, bad, n = {}, [], 0
    for fn, K, inner, dt, imp, idx in F.cases():
        x = fx.x(fn, K, inner, dt, imp)
        got = run(S, fn, torch.from_numpy(x).to(DEV), imp, idx).cpu().numpy()
        truth = fx.truth(fn, K, inner, imp, idx)
        ref = fx.ref(fn, K, inner, dt, imp, idx)
        assert got.shape == truth.shape, (fn, K, inner, dt, imp, idx, got.shape, truth.shape)
        r = F.ratio(got, truth, F.bound(fn, x, truth, imp, idx, dt))
        worst[(fn, dt)] = max(worst.get((fn, dt), 0.0), r)
        if not r <= fx.C:
            bad.append((fn, K, inner, dt, imp, idx, r))
        if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
                and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])):
            bad.append((fn, K, inner, dt, imp, idx, 'nan/inf pattern'))
        n += 1
    print('worst ratios (C = 1 bounds):', {f'{k[0]}/{k[1]}': round(v, 3) for k, v in sorted(worst.items())}, 'C =', fx.C)
    assert n > 1000
    assert not bad, bad[:10]


def test_special_values(S, fx):
    sp = fx.z['special_x']
    for fn in F.FUNCS:
        for imp in F.IMPLICIT:
            if fn == 'logsumexp' and imp[0] != imp[1]:
                continue
            for dt in F.DTYPES:
                x = torch.from_numpy(sp).to(TD[dt])
                if fn == 'logit':
                    x = x.abs().clamp_max(2.0) / 4
                got = run(S, fn, x.to(DEV), imp, 0).cpu().numpy()
                ref = fx.z[f'special_{fn}_{int(imp[0])}{int(imp[1])}_{dt}']
                assert np.array_equal(np.isnan(got), np.isnan(ref)), (fn, imp, dt, got[..., 0], ref[..., 0])
                assert np.array_equal(np.isinf(got), np.isinf(ref)), (fn, imp, dt)
                ok = np.isfinite(ref)
                assert np.allclose(got[ok], ref[ok], rtol=64 * F.EPS[dt], atol=64 * F.EPS[dt]), (fn, imp, dt)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_layouts_bit_for_bit(S, dt):
    """(N, K), (K, N) with dim=0, (B, K, X, Y) with dim=1, an odd base pointer and a side stream: identical bits"""
    g = torch.Generator().manual_seed(3)
    N = 4 * 5 * 24
    for K in range(1, 17):
        base = (torch.randn(N, K, generator=g, dtype=torch.float64) * 6).to(TD[dt]).to(DEV)
        for fn, imp, idx in itertools.product(('softmax', 'log_softmax', 'logit', 'logsumexp'), F.IMPLICIT, (0, -1)):
            if fn == 'logsumexp' and (imp[0] != imp[1] or idx):
                continue
            if K + imp[0] - imp[1] < 1:
                continue
            x = base if fn != 'logit' else torch.softmax(base, 1) * 0.9
            a = run(S, fn, x, imp, idx, 1)                                          # class-last
            b = run(S, fn, x.t().contiguous(), imp, idx, 0).t()                     # channel-first, 16-byte path
            x4 = x.reshape(4, 5, 24, K).permute(0, 3, 1, 2).contiguous()
            c = run(S, fn, x4, imp, idx, 1).permute(0, 2, 3, 1).reshape(N, -1)
            odd = x[:N - 1].t().contiguous()                                        # inner = N - 1: scalar path
            d = run(S, fn, odd, imp, idx, 0).t()
            buf = torch.empty(N * K + 1, dtype=x.dtype, device=DEV)
            buf[1:] = x.reshape(-1)
            e = run(S, fn, buf[1:].reshape(N, K), imp, idx, 1)                      # unaligned base
            f = run(S, fn, buf[1:].reshape(N, K).t().contiguous().t(), imp, idx, 1)  # permuted view of a contiguous tensor
            cf = buf[1:].reshape(K, N)                                              # channel-first at an odd base:
            assert same_bits(run(S, fn, cf, imp, idx, 0), run(S, fn, cf.clone(), imp, idx, 0)), (fn, K, imp, idx, 'cf odd')
            st = torch.cuda.Stream(DEV)
            st.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(st):
                h = run(S, fn, x, imp, idx, 1)
            st.synchronize()
            for name, o in (('dim0', b), ('bkxy', c), ('unaligned', e), ('view', f), ('stream', h)):
                assert same_bits(a, o), (fn, K, imp, idx, name)
            assert same_bits(a[:N - 1], d), (fn, K, imp, idx, 'odd inner')


def test_shapes_keepdim_negative_dim_and_indices(S):
    x = torch.randn(2, 5, 3, 4, device=DEV)
    assert S.softmax(x, 1).shape == (2, 5, 3, 4)
    assert S.softmax(x, 1, (True, False)).shape == (2, 6, 3, 4)
    assert S.softmax(x, 1, (False, True)).shape == (2, 4, 3, 4)
    assert S.softmax(x, -3, True).shape == (2, 5, 3, 4)
    assert torch.equal(S.softmax(x, -3, True), S.softmax(x, 1, True))
    assert S.logsumexp(x, 1).shape == (2, 3, 4) and S.logsumexp(x, -1, keepdim=True).shape == (2, 5, 3, 1)
    assert torch.allclose(S.logsumexp(x, 2), torch.logsumexp(x, 2), atol=1e-5)
    assert torch.allclose(S.softmax(x, 3), torch.softmax(x, 3), atol=1e-6)
    assert torch.allclose(S.log_softmax(x, 0), torch.log_softmax(x, 0), atol=1e-5)
    z = torch.zeros(2, 1, 3, 4, device=DEV)
    for idx in (0, 2, 5, -1, -3):                      # interior and negative positions of the added class
        j = idx % 6
        full = torch.softmax(torch.cat([x[:, :j], z, x[:, j:]], 1), 1)
        assert torch.allclose(S.softmax(x, 1, (True, False), idx), full, atol=1e-6), idx
        assert torch.allclose(S.softmax(x, 1, True, idx), torch.cat([full[:, :j], full[:, j + 1:]], 1), atol=1e-6)
        assert torch.allclose(S.log_softmax(x, 1, (True, False), idx), full.log(), atol=1e-5), idx
    for idx in (0, 2, -1):                             # class dropped from an explicit input
        j = idx % 5
        full = torch.softmax(x, 1)
        assert torch.allclose(S.softmax(x, 1, (False, True), idx), torch.cat([full[:, :j], full[:, j + 1:]], 1), atol=1e-6)
        lg = S.logit(full, 1, False, idx)
        assert torch.allclose(lg, full.log() - full.log()[:, j:j + 1], atol=1e-5)
        assert (lg[:, j] == 0).all()
    with pytest.raises(IndexError):
        S.softmax(x, 1, True, 6)
    with pytest.raises(IndexError):
        S.softmax(x, 1, False, -6)
    with pytest.raises(IndexError):
        S.softmax(x, 4)
    with pytest.raises(IndexError):
        S.softmax(torch.empty(3, 0, device=DEV), 1)
    assert S.softmax(torch.empty(0, 4, device=DEV), 1).shape == (0, 4)
    assert S.logsumexp(torch.empty(0, 4, device=DEV), 1).shape == (0,)
    assert S.softmax(torch.empty(3, 4, 0, device=DEV), 1, (True, False)).shape == (3, 5, 0)
    nc = torch.randn(6, 10, device=DEV)[:, ::2]        # not a view `_view3` can express: one contiguous()
    assert torch.allclose(S.softmax(nc, 1), torch.softmax(nc, 1), atol=1e-6)


def test_binary_case_and_inverse(S, fx):
    x = torch.randn(1000, 1, device=DEV, dtype=torch.float64) * 4
    assert torch.allclose(S.softmax(x, 1, True), torch.sigmoid(x), rtol=1e-14, atol=1e-300)
    p = torch.sigmoid(x)
    assert torch.allclose(S.logit(p, 1, True), torch.log(p) - torch.log1p(-p), rtol=1e-9, atol=1e-9)
    for dt in F.DTYPES:
        for K in (1, 3, 8, 16, 17, 40):
            x = (torch.randn(500, K, dtype=torch.float64) * 3).to(TD[dt])
            p = S.softmax(x.to(DEV), 1, True)
            back = S.logit(p, 1, True).cpu().numpy()
            pn = p.cpu().numpy()
            b = F.bound('logit', pn, back, (True, True), 0, dt)       # the logit bound at the computed p
            r = float((np.abs(back - x.numpy()) / b).max())
            print('logit(softmax(x)) - x over the logit bound:', dt, K, round(r, 3))
            assert r <= fx.C, (dt, K, r)


def test_more_than_2g_bytes(S, dev):
    """a field of more than 2^31 bytes: 64-bit addressing in both layouts"""
    from test_gpu_full_size import _need
    _need(dev, 8)
    n = (2 ** 31 + 2 ** 27) // 16
    x = torch.randn(n, 4, device=DEV)
    for xx, dim in ((x, 1), (x.view(4, n), 0)):
        p = S.softmax(xx, dim)
        ref = torch.softmax(xx, dim)
        assert torch.allclose(p, ref, atol=1e-6)
        del p, ref


def test_softmax_lse(S, fx):
    for K, inner, dt in itertools.product((3, 16, 40), F.INNERS, F.DTYPES):
        x = torch.from_numpy(fx.x('softmax', K, inner, dt, None)).to(DEV)
        w = torch.rand(x.shape[0], 1, x.shape[2], dtype=x.dtype, device=DEV)
        for imp in F.IMPLICIT:
            p, lse = S.softmax_lse(x, 1, None, imp)
            assert torch.equal(torch.nan_to_num(p), torch.nan_to_num(S.softmax(x, 1, imp, -1))), (K, inner, dt, imp)
            assert lse.dtype == torch.float64 and lse.dim() == 0
            tl = fx.truth('logsumexp', K, inner, (imp[0], imp[0]), 0)
            b = F.bound('logsumexp', fx.x('softmax', K, inner, dt, None), tl, (imp[0], imp[0]), 0, dt)
            assert abs(float(lse) - tl.sum()) <= fx.C * b.sum(), (K, inner, dt, imp)
            _, lw = S.softmax_lse(x, 1, w, imp)
            wn = w.cpu().numpy().astype(np.float64)
            assert abs(float(lw) - (tl * wn).sum()) <= fx.C * (b * wn).sum() + F.EPS[dt] * np.abs(tl * wn).sum(), \
                (K, inner, dt, imp)


@pytest.mark.parametrize('fn', ['softmax', 'log_softmax', 'logit', 'logsumexp', 'softmax_lse'])
def test_gradcheck(S, fn):
    g = torch.Generator().manual_seed(11)
    for imp in F.IMPLICIT:
        for idx in (0, 1, -1):
            if fn in ('logsumexp', 'softmax_lse') and idx != 0:
                continue
            for shape, dim in (((4, 3), 1), ((2, 3, 5), 1)):
                x = torch.randn(shape, dtype=torch.float64, generator=g)
                if fn == 'logit':
                    x = torch.softmax(torch.cat([x, torch.zeros_like(x[:, :1])], 1), 1)[:, :3]
                    if not imp[0]:
                        x = x + 0.1
                x = x.to(DEV).requires_grad_()
                if fn == 'logsumexp':
                    if imp[0] != imp[1]:
                        continue
                    f = lambda t: S.logsumexp(t, dim, False, imp[0])                      # noqa: E731
                elif fn == 'softmax_lse':
                    w = torch.rand(shape[:1] + (1,) + shape[2:], dtype=torch.float64, device=DEV)
                    f = lambda t: S.softmax_lse(t, dim, w, imp)                            # noqa: E731
                else:
                    f = lambda t: getattr(S, fn)(t, dim, imp, idx)                         # noqa: E731
                assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-7, rtol=1e-6), (fn, imp, idx, shape)


def test_gradients_against_fixture_and_float32(S, fx):
    for inner in (1, 7):
        x = torch.from_numpy(fx.z[f'x_3_{inner}']).double().to(DEV)
        for tag, imp in (('e', (False, False)), ('i', (True, True))):
            for fn in ('softmax', 'log_softmax', 'logsumexp'):
                go = torch.from_numpy(fx.z[f'gout_{fn}_{tag}_{inner}']).to(DEV)
                want = fx.z[f'gin_{fn}_{tag}_{inner}']
                xr = x.clone().requires_grad_()
                (gx,) = torch.autograd.grad(run(S, fn, xr, imp, 0), xr, go)
                scale = np.abs(want).max() + np.abs(go.cpu().numpy()).max()
                assert np.abs(gx.cpu().numpy() - want).max() <= fx.C * F.EPS['f64'] * 16 * scale, (fn, tag, inner)
    # float32 gradients against float64 ones (grad_bound)
    g = torch.Generator().manual_seed(5)
    for K, imp, idx in itertools.product((3, 16, 17, 40), F.IMPLICIT, (0, -1)):
        x64 = (torch.randn(300, K, 7, dtype=torch.float64, generator=g) * 3).float().double().to(DEV)
        for fn in ('softmax', 'log_softmax', 'logsumexp'):
            if fn == 'logsumexp' and (imp[0] != imp[1] or idx):
                continue
            outs = {}
            for dt in (torch.float64, torch.float32):
                xr = x64.to(dt).requires_grad_()
                y = run(S, fn, xr, imp, idx)
                go = torch.linspace(-1, 1, y.numel(), dtype=torch.float64, device=DEV).reshape(y.shape).float().double()
                outs[dt] = torch.autograd.grad(y, xr, go.to(dt))[0].double()
            bnd = grad_bound(fn, x64, go, imp, idx, 'f32', fx.C)
            assert ((outs[torch.float32] - outs[torch.float64]).abs() <= bnd).all(), (fn, K, imp, idx)


def test_one_saved_tensor_per_function(S):
    x = torch.randn(10, 4, device=DEV, requires_grad=True)
    for y in (S.softmax(x, 1, True), S.log_softmax(x, 1, (True, False)), S.logsumexp(x, 1, True, True)):
        saved = [a for a in dir(y.grad_fn) if a.startswith('_saved')]
        assert type(y.grad_fn).__name__.endswith('FnBackward') and len(y.grad_fn.saved_tensors) == 1, (y.grad_fn, saved)


def test_runtime_k_and_torch_route_agree(S, fx):
    """K = 16 (registers), 17..48 (class sweeps) and 49+ (torch ops) within the bounds of one another"""
    from nitorch_fastmath_amd import simplex as M
    assert (M.REGISTER_MAX_KP, M.MAX_K) == (17, 48)
    g = torch.Generator().manual_seed(9)
    for dt in F.DTYPES:
        for K, inner in itertools.product((16, 17, 33, 48, 49, 70), (1, 12, 7)):
            x = (torch.randn(50, K, inner, dtype=torch.float64, generator=g) * 5).to(TD[dt])
            xd = x.to(DEV)
            for imp, idx in itertools.product(F.IMPLICIT, (0, 5, -1)):
                for fn in ('softmax', 'log_softmax', 'logsumexp'):
                    if fn == 'logsumexp' and (imp[0] != imp[1] or idx):
                        continue
                    got = run(S, fn, xd, imp, idx).cpu().numpy()
                    kp = K + imp[0]
                    j = idx % kp
                    z = x.double()
                    if imp[0]:
                        z = torch.cat([z[:, :j], torch.zeros(50, 1, inner, dtype=torch.float64), z[:, j:]], 1)
                    t = {'softmax': torch.softmax(z, 1), 'log_softmax': torch.log_softmax(z, 1),
                         'logsumexp': torch.logsumexp(z, 1, keepdim=True)}[fn]
                    if imp[1] and fn != 'logsumexp':
                        t = torch.cat([t[:, :j], t[:, j + 1:]], 1)
                    t = t.numpy()
                    b = F.bound(fn, x.numpy(), t, imp, idx, dt)
                    assert F.ratio(got, t, b) <= fx.C, (dt, K, inner, fn, imp, idx, F.ratio(got, t, b))
            # backward: runtime-K kernels against float64 autograd of the torch route (grad_bound)
            for fn in ('softmax', 'log_softmax', 'logsumexp'):
                imp = (True, False) if fn != 'logsumexp' else (True, True)
                xr = xd.clone().requires_grad_()
                y = run(S, fn, xr, imp, 0)
                go = torch.linspace(-1, 1, y.numel(), dtype=torch.float64, device=DEV).reshape(y.shape).float().double()
                (gx,) = torch.autograd.grad(y, xr, go.to(y.dtype))
                z = torch.cat([torch.zeros(50, 1, inner, dtype=torch.float64), x.double()], 1).requires_grad_()
                t = {'softmax': torch.softmax(z, 1), 'log_softmax': torch.log_softmax(z, 1),
                     'logsumexp': torch.logsumexp(z, 1, keepdim=True)}[fn]
                (gz,) = torch.autograd.grad(t, z, go.cpu())
                bnd = grad_bound(fn, xd.double(), go, imp, 0, dt, fx.C).cpu()
                assert ((gx.cpu().double() - gz[:, 1:]).abs() <= bnd).all(), (dt, K, inner, fn)
