"""`sym.sym_funm` on the GPU: per-record conditioning bounds of the result and of the gradient against the model of
tests/_symfun_ref.py, every layout against the contiguous call bit for bit, the domain rule, consistency between the
functions, the torch route above the compiled caps, graph capture, and the computation dtype."""
import numpy as np
import pytest
import torch
import _symfun_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'f64': torch.float64}
ORDERS = (1, 2, 3, 4, 6, 8)


def S():
    from nitorch_fastmath_amd import sym
    return sym


def cap(dn, bwd):
    return S()._funm_cap(TD[dn], bwd)


def run(dev, comp, fn, p=None, vmin=None, g=None, **kw):
    """(result, gradient or None) as numpy arrays"""
    x = torch.as_tensor(np.array(comp), device=dev)
    if g is None:
        return S().sym_funm(x, fn, p=p, min=vmin, **kw).cpu().numpy(), None
    x.requires_grad_(True)
    y = S().sym_funm(x, fn, p=p, min=vmin, **kw)
    y.backward(torch.as_tensor(np.array(g), device=dev))
    return y.detach().cpu().numpy(), x.grad.cpu().numpy()


def report(tag, cells, ratio):
    for fam, sl in cells.items():
        print(f'{tag} {fam}: {np.nanmax(ratio[sl]):.2f} (of {R.C})')


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize('fn', R.FUNCS)
@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_forward_and_backward_bounds(dev, dn, n, fn):
    """per record, every family: ||Y^ - Y|| <= 16 n eps (L ||A|| + ||Y||) and
    ||S^ - S|| <= 16 n eps (M2 ||A|| + L) ||G|| (exp: n + max|l|), finite everywhere -- isotropic, repeated and
    cluster included.  Orders above the backward cap take the kernel forward and the torch route backward."""
    if dn == 'f64':
        assert R.high_ok()
    assert n <= cap(dn, 0)
    comp, cells = R.batch(dn, n, fn)
    g = R.cotangent(dn, n)
    p, vmin = R.fn_args(fn)
    mod = R.truth(dn, n, fn)
    y, gx = run(dev, comp, fn, p, vmin, g)
    assert np.isfinite(y).all() and np.isfinite(gx).all()
    rf, rb = R.forward_ratio(dn, fn, mod, y), R.backward_ratio(dn, fn, mod, g, gx)
    report(f'{fn} {dn} n={n} forward', cells, rf)
    report(f'{fn} {dn} n={n} backward', cells, rb)
    assert rf.max() <= R.C, (rf.max(), int(rf.argmax()))
    assert rb.max() <= R.C, (rb.max(), int(rb.argmax()))


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(dev, x):
    """{name: a tensor equal to x in another layout}"""
    nb, K = x.shape
    out = {}
    out['channel_first'] = x.t().contiguous().t()                                   # (K, n) storage viewed as (n, K)
    wide = torch.zeros(nb, K + 3, device=dev, dtype=x.dtype)
    wide[:, 1:K + 1] = x
    out['padded'] = wide[:, 1:K + 1]                                                 # a slice of a wider last dim
    flat = torch.zeros(nb * K + 1, device=dev, dtype=x.dtype)
    flat[1:] = x.reshape(-1)
    out['odd_offset'] = flat[1:].view(nb, K)                                         # base at an odd element offset
    return out


@pytest.mark.parametrize('n', [3, 6, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_layouts_give_the_same_bits(dev, dn, n):
    sym = S()
    comp, _ = R.batch(dn, n, 'log')
    x = torch.as_tensor(np.array(comp), device=dev)
    g = torch.as_tensor(np.array(R.cotangent(dn, n)), device=dev)
    bwd_kernel = n <= cap(dn, 1)

    def both(xx, gg):
        xx = xx.detach().requires_grad_(True)
        y = sym.sym_logm(xx)
        y.backward(gg)
        return y.detach(), xx.grad

    y0, g0 = both(x, g)
    for name, xl in _layouts(dev, x).items():
        gl = _layouts(dev, g)[name]
        y, gx = both(xl, gl)
        assert torch.equal(y, y0), name
        if bwd_kernel:
            assert torch.equal(gx, g0), name
        plain = sym.sym_logm(xl)
        assert torch.equal(plain, y0), name
        if name == 'channel_first':
            assert plain.stride() == xl.stride() and y.stride() == xl.stride()        # the layout is handed on
            if bwd_kernel:
                assert sym._funm_backward(xl, gl, 1, 0.0, None, None).stride() == xl.stride()
    # a broadcast batch (stride 0): one record for every element
    xb = x[5:6].expand(64, -1)
    yb = sym.sym_logm(xb)
    assert torch.equal(yb, y0[5:6].expand(64, -1))
    if bwd_kernel:
        gb = sym._funm_backward(xb, g[:64], 1, 0.0, None, None)
        assert torch.equal(gb, sym._funm_backward(xb.contiguous(), g[:64], 1, 0.0, None, None))
        # a broadcast cotangent (what .sum().backward() sends)
        xr = x.detach().requires_grad_(True)
        sym.sym_logm(xr).sum().backward()
        assert torch.equal(xr.grad, sym._funm_backward(x, torch.ones_like(x), 1, 0.0, None, None))
    # out= given, and out=mat (in place)
    out = torch.empty_like(x)
    assert sym.sym_logm(x, out=out) is out and torch.equal(out, y0)
    xi = x.clone()
    assert sym.sym_logm(xi, out=xi) is xi and torch.equal(xi, y0)
    xc = _layouts(dev, x)['channel_first'].clone(memory_format=torch.preserve_format)
    sym.sym_logm(xc, out=xc)
    assert torch.equal(xc, y0)


# ------------------------------------------------------------------------------------------------ the domain
@pytest.mark.parametrize('fn', ['log', 'sqrt', 'rsqrt', 'pow'])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_domain_violations_are_nan_records(dev, dn, fn):
    n = 3
    comp = np.array(R.batch(dn, n, fn)[0])
    g = R.cotangent(dn, n)
    p, _ = R.fn_args(fn)
    y0, g0 = run(dev, comp, fn, p, None, g)
    bad = np.array(comp)
    neg, nan = 100, 171                       # inside the first tile, between good records
    bad[neg] = R.pack(np.diag([1.0, -0.5, 2.0])[None])[0]
    bad[nan, 4] = np.nan
    y, gx = run(dev, bad, fn, p, None, g)
    others = np.ones(len(comp), bool)
    others[[neg, nan]] = False
    for r, r0 in ((y, y0), (gx, g0)):
        assert np.isnan(r[[neg, nan]]).all()
        assert np.array_equal(r[others], r0[others])
    # the same input with a clamp: only the record with the NaN entry is NaN, and the bound holds
    y, gx = run(dev, bad, fn, p, 1e-3, g)
    others[neg] = True
    assert np.isnan(y[nan]).all() and np.isnan(gx[nan]).all()
    assert np.isfinite(y[others]).all() and np.isfinite(gx[others]).all()
    mod = R.model(dn, fn, bad[others], p, 1e-3, g[others])
    rf, rb = R.forward_ratio(dn, fn, mod, y[others]), R.backward_ratio(dn, fn, mod, g[others], gx[others])
    print(f'{fn} {dn} min=1e-3: forward {rf.max():.2f} backward {rb.max():.2f} (of {R.C})')
    assert rf.max() <= R.C and rb.max() <= R.C


# ------------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize('n', [3, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_functions_are_consistent(dev, dn, n):
    """sqrt against pow(0.5), rsqrt against pow(-0.5), exp(log(A)) against A: within the sum of the two bounds"""
    sym = S()
    eps = R.eps_of(dn)
    hp = R.HP[dn]
    comp, _ = R.batch(dn, n, 'pow')                      # no scaled records: pow is not meant for them
    x = torch.as_tensor(np.array(comp), device=dev)
    for fn, p in (('sqrt', 0.5), ('rsqrt', -0.5)):
        a = sym.sym_funm(x, fn).cpu().numpy()
        b = sym.sym_powm(x, p).cpu().numpy()
        ma, mb = R.model(dn, fn, comp), R.model(dn, 'pow', comp, p)
        bound = R.C * n * eps * (ma['L'] * ma['normA'] + ma['normY'] + mb['L'] * mb['normA'] + mb['normY'])
        err = R._fro(R.unpack(a.astype(hp), n) - R.unpack(b.astype(hp), n))
        assert (err <= bound).all(), (fn, (err / bound).max())
    lg = sym.sym_logm(x)
    back = sym.sym_expm(lg).cpu().numpy()
    lgn = lg.cpu().numpy()
    ml, me = R.model(dn, 'log', comp), R.model(dn, 'exp', lgn)
    # the error of the logarithm goes through exp: its Lipschitz constant there is L of the second model
    bound = R.C * eps * (n * (ml['L'] * ml['normA'] + ml['normY']) * me['L']
                         + (n + me['lam_max']) * (me['L'] * me['normA'] + me['normY']))
    err = R._fro(R.unpack(back.astype(hp), n) - R.unpack(np.asarray(comp).astype(hp), n))
    assert (err <= bound).all(), (err / bound).max()


# ------------------------------------------------------------------------------------------------ the torch route
@pytest.mark.parametrize('fn', ['log', 'rsqrt'])
@pytest.mark.parametrize('n', [9, 16])
def test_orders_above_the_caps_take_the_torch_route(dev, n, fn):
    assert R.high_ok() and n > cap('f64', 0)
    nb = 7 * 8
    comp, cells = R.batch('f64', n, fn, nb=nb)
    g = R.cotangent('f64', n, nb=nb)
    mod = R.model('f64', fn, comp, None, None, g)
    y, gx = run(dev, comp, fn, None, None, g)
    rf, rb = R.forward_ratio('f64', fn, mod, y), R.backward_ratio('f64', fn, mod, g, gx)
    print(f'{fn} n={n}: forward {rf.max():.2f} backward {rb.max():.2f} (of {R.C})')
    assert rf.max() <= R.C and rb.max() <= R.C
    out = torch.empty(nb, comp.shape[1], device=dev, dtype=torch.float64)
    assert S().sym_funm(torch.as_tensor(np.array(comp), device=dev), fn, out=out) is out
    assert np.array_equal(out.cpu().numpy(), y)


def test_between_the_caps_kernel_forward_torch_backward(dev):
    """the orders between the backward cap and the forward cap: the forward is the kernel's (its bits), the gradient
    is the torch route's (test_forward_and_backward_bounds holds it to the bound for every function there)"""
    from nitorch_fastmath_amd import _symfun
    for dn in ('f32', 'f64'):
        for n in range(cap(dn, 1) + 1, cap(dn, 0) + 1):
            comp, _ = R.batch(dn, n, 'log')
            g = R.cotangent(dn, n)
            y, gx = run(dev, comp, 'log', None, None, g)
            y_plain, _ = run(dev, comp, 'log')
            assert np.array_equal(y, y_plain)
            want = _symfun.backward(torch.as_tensor(np.array(comp), device=dev),
                                    torch.as_tensor(np.array(g), device=dev), 1)
            assert np.array_equal(gx, want.cpu().numpy())


# ------------------------------------------------------------------------------------------------ graphs, dtype
def test_forward_and_backward_capture_in_a_graph(dev):
    """forward plus backward (through autograd) captured in one graph on one stream, replayed twice on refreshed
    inputs: the bits of the eager call"""
    sym = S()
    n = 3
    comp, _ = R.batch('f32', n, 'pow')
    x = torch.as_tensor(np.array(comp), device=dev).requires_grad_(True)
    g = torch.as_tensor(np.array(R.cotangent('f32', n)), device=dev)

    def eager(xx, gg):
        xx = xx.detach().clone().requires_grad_(True)
        yy = sym.sym_powm(xx, 1.7, min=0.6)
        yy.backward(gg)
        return yy.detach(), xx.grad

    side = torch.cuda.Stream(device=dev)         # warm-up outside the capture (module load, autograd's buffers)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        sym.sym_powm(x, 1.7, min=0.6).backward(g)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = sym.sym_powm(x, 1.7, min=0.6)
        y.backward(g)
    for k in range(2):
        with torch.no_grad():
            x.mul_(1.25)
            g.mul_(-0.5)
        graph.replay()
        torch.cuda.synchronize()
        ye, ge = eager(x, g)
        assert torch.equal(y.detach(), ye) and torch.equal(x.grad, ge), k


def test_dtype_argument_computes_in_float64(dev):
    sym = S()
    comp, _ = R.batch('f32', 4, 'log')
    x32 = torch.as_tensor(np.array(comp), device=dev)
    y = sym.sym_logm(x32, dtype=torch.float64)
    assert y.dtype == torch.float64 and torch.equal(y, sym.sym_logm(x32.double()))
    xr = x32.clone().requires_grad_(True)
    sym.sym_logm(xr, dtype=torch.float64).sum().backward()
    assert xr.grad.dtype == torch.float32
    x64 = x32.double().requires_grad_(True)
    sym.sym_logm(x64).sum().backward()
    assert torch.equal(xr.grad, x64.grad.float())
