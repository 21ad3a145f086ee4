"""`sym.sym_eigvals` / `sym.sym_eigh` on the GPU: the per-record bars of tests/_eig_ref.py on its whole batch, the
order and the sign rule on the output, the gradients within the conditioning bounds of tests/_symeig_ref.py, the
identities on degenerate spectra, every layout against the contiguous call bit for bit, the NaN rule, the torch route
above the compiled caps and graph capture."""
import numpy as np
import pytest
import torch
import _eig_ref as E
import _symeig_ref as Q
import _symfun_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'f64': torch.float64}
ORDERS = (2, 3, 4, 5, 6, 8)
VALUES, VECTORS, VALUES_BACKWARD, BACKWARD = range(4)


def S():
    from nitorch_fastmath_amd import sym
    return sym


def cap(dn, op):
    return S()._eigh_cap(TD[dn], op)


def dev_of(x, dev):
    return torch.as_tensor(np.array(x), device=dev)


def grads(dev, comp, order, gl=None, gv=None):
    """(values, vectors, gradient) as numpy arrays for the cotangents given"""
    x = dev_of(comp, dev).requires_grad_(True)
    lam, V = S().sym_eigh(x, order=order)
    outs = [t for t, g in ((lam, gl), (V, gv)) if g is not None]
    torch.autograd.backward(outs, [dev_of(g, dev) for g in (gl, gv) if g is not None])
    return lam.detach().cpu().numpy(), V.detach().cpu().numpy(), x.grad.cpu().numpy()


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_forward_meets_the_bars_in_every_cell(dev, dn, n):
    """the whole `_eig_ref.batch`: every family, the scale sweep, subnormals, specials, plain and shuffled; all three
    metrics <= C in every cell (the FAST sweeps have no exclusions); order, signs and the relations between orders"""
    sym = S()
    assert n <= cap(dn, VALUES) and n <= cap(dn, VECTORS)
    a = E.batch(dn, n)[0]
    x = dev_of(R.pack(a), dev)
    vals = sym.sym_eigvals(x)
    lam, V = sym.sym_eigh(x)
    vals_n, lam_n, vecs = vals.cpu().numpy(), lam.cpu().numpy(), V.cpu().numpy()
    worst = E.per_cell(dn, n, E.judge(dn, n, vals_n, lam_n, vecs))
    for m in E.METRICS:
        c = max((c for c, mm in worst if mm == m), key=lambda c: worst[(c, m)])
        print(f'{dn} n={n} {m}: worst {worst[(c, m)]:.2f} in {c} (of {E.C})')
    assert not E.exceeding(dn, n, worst), sorted(E.exceeding(dn, n, worst))
    r = E.same_value_set(dn, n, vals_n, lam_n)
    assert r.max() <= 2 * E.C, float(r.max())
    out = {'ascending': (vals_n, lam_n, vecs)}
    for order in ('descending', 'abs'):
        l2, V2 = sym.sym_eigh(x, order=order)
        out[order] = (sym.sym_eigvals(x, order=order).cpu().numpy(), l2.cpu().numpy(), V2.cpu().numpy())
    for order, (v, l, u) in out.items():
        assert np.isfinite(v).all() and np.isfinite(l).all() and np.isfinite(u).all()
        assert Q.is_sorted(v, order).all() and Q.is_sorted(l, order).all(), order
        assert Q.signs_ok(u).all(), order
    # 'descending' is the bit-exact reverse of 'ascending', 'abs' a permutation of the same bits
    for k in (0, 1):
        asc = out['ascending'][k]
        assert np.array_equal(out['descending'][k].view(np.uint8), asc[:, ::-1].copy().view(np.uint8))
        bits = asc.view(np.uint32 if dn == 'f32' else np.uint64)
        assert np.array_equal(np.sort(out['abs'][k].view(bits.dtype), -1), np.sort(bits, -1))
    # the columns travel with their values: the residual of the other orders
    for order in ('descending', 'abs'):
        v, l, u = out[order]
        res, orth = E.judge_vectors(dn, n, l, u)
        assert res.max() <= E.C and orth.max() <= E.C, (order, float(res.max()), float(orth.max()))


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_gradients_within_the_bounds(dev, dn, n):
    """'normal' and 'wilk': the cotangent of the values alone, of the vectors alone, and both; no record excluded.
    Orders above a backward cap take the kernel forward and the torch route backward (the split route)."""
    if dn == 'f64':
        assert R.high_ok()
    assert n <= cap(dn, VECTORS)
    full, comp, cells = Q.grad_batch(dn, n)
    gl, gv = Q.cotangents(dn, n, len(full))
    order = 'abs' if n == 4 else 'ascending'
    worst = {}
    mod = None
    for name, a, b in (('values', gl, None), ('vectors', None, gv), ('both', gl, gv)):
        _, vecs, gx = grads(dev, comp, order, a, b)
        if mod is None:
            mod = Q.model(dn, full, order, vecs, gl, gv, hp=Q._eigh_hp(dn, n))
            assert Q.judged(dn, n, mod).all(), 'no record of these cells may be excluded'
        r = Q.grad_ratio(dn, n, mod, gx, a, b)
        worst[name] = {c: float(r[sl].max()) for c, sl in cells.items()}
    print(f'{dn} n={n} {order}: {worst} (of {Q.C})')
    assert max(max(v.values()) for v in worst.values()) <= Q.C, worst
    # the values' gradient of sym_eigvals is the one of sym_eigh
    x = dev_of(comp, dev).requires_grad_(True)
    S().sym_eigvals(x, order=order).backward(dev_of(gl, dev))
    assert np.array_equal(x.grad.cpu().numpy(), grads(dev, comp, order, gl, None)[2])


def test_one_order_above_a_backward_cap_takes_the_split_route(dev):
    from nitorch_fastmath_amd import _symeig
    split = [(dn, n) for dn in ('f32', 'f64') for n in range(cap(dn, BACKWARD) + 1, cap(dn, VECTORS) + 1)]
    assert split, 'every order with a forward kernel has a backward kernel: nothing takes the split route'
    for dn, n in split[:1]:
        assert n in ORDERS                      # test_gradients_within_the_bounds holds it to the bounds
        full, comp, _ = Q.grad_batch(dn, n)
        gl, gv = Q.cotangents(dn, n, len(full))
        lam, V, gx = grads(dev, comp, 'ascending', gl, gv)
        bad = torch.zeros(len(comp), dtype=torch.bool, device=dev)
        want = _symeig.backward_from(dev_of(lam, dev), dev_of(V, dev), bad, dev_of(gl, dev), dev_of(gv, dev))
        assert np.array_equal(gx, want.cpu().numpy())


@pytest.mark.parametrize('n', [3, 6, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_degenerate_spectra_give_finite_gradients_and_identities(dev, dn, n):
    comp, cells = R.batch(dn, n, 'log')
    gl, gv = Q.cotangents(dn, n, len(comp))
    for fam in ('isotropic', 'repeated', 'cluster'):
        sl = cells[fam]
        for a, b in ((gl[sl], None), (None, gv[sl]), (gl[sl], gv[sl])):
            lam, V, gx = grads(dev, comp[sl], 'ascending', a, b)
            assert np.isfinite(lam).all() and np.isfinite(V).all() and np.isfinite(gx).all(), (fam, a is None, b is None)
        # gl = 1: S = V V^T = I (rows' and columns' orthogonality defects share a 2-norm: n times the max-norm bar)
        _, _, gx = grads(dev, comp[sl], 'ascending', np.ones_like(gl[sl]), None)
        s = R.unpack(gx, n, off=0.5)
        err = np.abs(s - np.eye(n)).max()
        print(f'{dn} n={n} {fam}: |S - I|_max {err / (n * n * R.eps_of(dn)):.2f} n^2 eps (of {Q.C})')
        assert err <= Q.C * n * n * R.eps_of(dn), fam


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(dev, x):
    """{name: a tensor equal to x in another layout} (the recipe of tests/test_gpu_symfun.py)"""
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
    comp = Q.grad_batch(dn, n)[1]
    x = dev_of(comp, dev)
    nb = len(x)
    gl_np, gv_np = Q.cotangents(dn, n, nb)
    gl, gv = dev_of(gl_np, dev), dev_of(gv_np, dev)
    full_kernel = n <= cap(dn, BACKWARD)

    def both(xx, a, b):
        xx = xx.detach().requires_grad_(True)
        lam, V = sym.sym_eigh(xx, order='abs')
        torch.autograd.backward([lam, V], [a, b])
        return lam.detach(), V.detach(), xx.grad

    def vals_only(xx, a):
        xx = xx.detach().requires_grad_(True)
        v = sym.sym_eigvals(xx, order='abs')
        v.backward(a)
        return v.detach(), xx.grad

    l0, V0, g0 = both(x, gl, gv)
    v0, gv0 = vals_only(x, gl)
    for name, xl in _layouts(dev, x).items():
        gll = _layouts(dev, gl)[name]
        gvl = _layouts(dev, gv.reshape(nb, n * n))[name].unflatten(-1, (n, n))
        lam, V, gx = both(xl, gll, gvl)
        assert torch.equal(lam, l0) and torch.equal(V, V0), name
        if full_kernel:
            assert torch.equal(gx, g0), name
        v, gxv = vals_only(xl, gll)
        assert torch.equal(v, v0) and torch.equal(gxv, gv0), name
        plain = sym.sym_eigvals(xl, order='abs')
        assert torch.equal(plain, v0), name
        if name == 'channel_first':                                                  # the layout is handed on
            assert plain.stride() == (1, nb) and v.stride() == (1, nb)
            assert sym._eigh_backward(xl, gll, None, 2, None).stride() == xl.stride()
            if full_kernel:
                assert sym._eigh_backward(xl, gll, gvl, 2, None).stride() == xl.stride()
    # a broadcast batch (stride 0): one record for every element
    xb = x[5:6].expand(64, -1)
    assert torch.equal(sym.sym_eigvals(xb, order='abs'), v0[5:6].expand(64, -1))
    lb, Vb = sym.sym_eigh(xb, order='abs')
    assert torch.equal(lb, l0[5:6].expand(64, -1)) and torch.equal(Vb, V0[5:6].expand(64, -1, -1))
    assert torch.equal(sym._eigh_backward(xb, gl[:64], None, 2, None),
                       sym._eigh_backward(xb.contiguous(), gl[:64], None, 2, None))
    # a broadcast cotangent (what .sum().backward() sends), and an absent one
    xr = x.detach().requires_grad_(True)
    sym.sym_eigvals(xr, order='abs').sum().backward()
    assert torch.equal(xr.grad, sym._eigh_backward(x, torch.ones_like(gl), None, 2, None))
    if full_kernel:
        xr = x.detach().requires_grad_(True)
        sym.sym_eigh(xr, order='abs')[1].backward(gv)
        assert torch.equal(xr.grad, sym._eigh_backward(x, torch.zeros_like(gl), gv, 2, None))
    # out= given
    out = torch.empty(nb, n, device=dev, dtype=x.dtype)
    assert sym.sym_eigvals(x, order='abs', out=out) is out and torch.equal(out, v0)
    wide = torch.zeros(nb, n + 2, device=dev, dtype=x.dtype)
    sym.sym_eigvals(x, order='abs', out=wide[:, 1:n + 1])
    assert torch.equal(wide[:, 1:n + 1], v0) and (wide[:, 0] == 0).all() and (wide[:, -1] == 0).all()


# ------------------------------------------------------------------------------------------------ the NaN rule
@pytest.mark.parametrize('n', [3, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_bad_records_are_nan_and_their_neighbours_untouched(dev, dn, n):
    comp = np.array(Q.grad_batch(dn, n)[1][:5])
    comp[1, n + 1] = np.nan
    comp[3, 0] = np.inf
    gl, gv = Q.cotangents(dn, n, 5)
    good = [0, 2, 4]
    vals = S().sym_eigvals(dev_of(comp, dev)).cpu().numpy()
    lam, V, gx = grads(dev, comp, 'ascending', gl, gv)
    x = dev_of(comp, dev).requires_grad_(True)
    S().sym_eigvals(x).backward(dev_of(gl, dev))
    gxv = x.grad.cpu().numpy()
    for r in (vals, lam, V.reshape(5, -1), gx, gxv):
        assert np.isnan(r[[1, 3]]).all() and np.isfinite(r[good]).all()
    lam2, V2, gx2 = grads(dev, comp[good], 'ascending', gl[good], gv[good])
    assert np.array_equal(lam[good], lam2) and np.array_equal(V[good], V2) and np.array_equal(gx[good], gx2)
    assert np.array_equal(vals[good], S().sym_eigvals(dev_of(comp[good], dev)).cpu().numpy())


# ------------------------------------------------------------------------------------------------ above the caps
@pytest.mark.parametrize('n', [9, 16])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_orders_above_the_caps_take_the_torch_route(dev, dn, n):
    assert n > cap(dn, VALUES)
    a = E.batch(dn, n)[0]
    keep = np.concatenate([E.batch(dn, n)[1][c] for c in E.FAMILIES])          # unit scale: torch's eigh does not scale
    a = a[keep]
    x = dev_of(R.pack(a), dev)
    vals = S().sym_eigvals(x, order='abs')
    lam, V = S().sym_eigh(x, order='abs')
    vals_n, lam_n, vecs = vals.cpu().numpy(), lam.cpu().numpy(), V.cpu().numpy()
    E.assert_records_within(dn, n, a, vals_n, lam_n, vecs)
    assert Q.is_sorted(vals_n, 'abs').all() and Q.is_sorted(lam_n, 'abs').all() and Q.signs_ok(vecs).all()
    xr = x[:64].clone().requires_grad_(True)
    l2, V2 = S().sym_eigh(xr)
    (l2.sum() + (V2 * V2).sum()).backward()
    assert torch.isfinite(xr.grad).all()


# ------------------------------------------------------------------------------------------------ graphs
def test_forward_and_backward_capture_in_a_graph(dev):
    """forward plus backward (through autograd) captured in one graph on one stream, replayed twice on refreshed
    inputs: the bits of the eager call"""
    sym = S()
    n = 3
    comp = Q.grad_batch('f32', n)[1]
    x = dev_of(comp, dev).requires_grad_(True)
    gl_np, gv_np = Q.cotangents('f32', n, len(comp))
    gl, gv = dev_of(gl_np, dev), dev_of(gv_np, dev)

    def run(xx):
        lam, V = sym.sym_eigh(xx, order='descending')
        torch.autograd.backward([lam, V], [gl, gv])
        return lam, V

    def eager(xx):
        xx = xx.detach().clone().requires_grad_(True)
        lam, V = run(xx)
        return lam.detach(), V.detach(), xx.grad

    side = torch.cuda.Stream(device=dev)         # warm-up outside the capture (module load, autograd's buffers)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(x)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lam, V = run(x)
    for k in range(2):
        with torch.no_grad():
            x.mul_(1.25)
            gl.mul_(-0.5)
            gv.mul_(2.0)
        graph.replay()
        torch.cuda.synchronize()
        le, Ve, ge = eager(x)
        assert torch.equal(lam.detach(), le) and torch.equal(V.detach(), Ve) and torch.equal(x.grad, ge), k


def test_dtype_argument_computes_in_float64(dev):
    sym = S()
    x32 = dev_of(Q.grad_batch('f32', 4)[1], dev)
    v = sym.sym_eigvals(x32, dtype=torch.float64)
    assert v.dtype == torch.float64 and torch.equal(v, sym.sym_eigvals(x32.double()))
    xr = x32.clone().requires_grad_(True)
    lam, V = sym.sym_eigh(xr, dtype=torch.float64)
    assert lam.dtype == torch.float64 and V.dtype == torch.float64
    (lam.sum() + V.sum()).backward()
    assert xr.grad.dtype == torch.float32 and torch.isfinite(xr.grad).all()
