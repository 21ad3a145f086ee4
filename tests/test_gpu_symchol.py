"""The Cholesky functions of `sym` on the GPU (sym_chol, sym_chol_apply, sym_logdet, sym_mahalanobis,
sym_gauss_logpdf): every op, forward and backward, on the whole batch of tests/_symchol_ref.py against its per-record
bounds; every layout against the contiguous call bit for bit; the consistency of the ops with each other; the
bad-record rule; the torch composition above the compiled caps; graph capture and the empty batch."""
import numpy as np
import pytest
import torch
import _symchol_ref as C
import _symfun_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'f64': torch.float64}
FACTOR, APPLY, SCALAR, BACKWARD = range(4)
FORWARD_OPS = ('factor',) + C.APPLY + C.SCALARS


def S():
    from nitorch_fastmath_amd import sym
    return sym


def dev_of(x, dev):
    return torch.as_tensor(np.array(x), device=dev)


def forward(op, mat, vec, **kw):
    sym = S()
    if op == 'factor':
        return sym.sym_chol(mat, **kw)
    if op in C.APPLY:
        return sym.sym_chol_apply(mat, vec, op, **kw)
    if op == 'logdet':
        return sym.sym_logdet(mat, **kw)
    if op in ('maha', 'maha_sqrt'):
        return sym.sym_mahalanobis(mat, vec, squared=op == 'maha', **kw)
    return sym.sym_gauss_logpdf(mat, vec, **kw)


def backward(op, mat, vec, g):
    """(value, packed gradient [K | n]; logdet: [K]) through autograd"""
    a = mat.detach().requires_grad_(True)
    v = vec.detach().requires_grad_(True)
    res = forward(op, a, v)
    res.backward(g)
    return res.detach(), (a.grad if op == 'logdet' else torch.cat([a.grad, v.grad], -1))


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_every_op_meets_its_bounds(dev, dn, n):
    """forward and backward on the 1200 records: every ratio <= 1 in every cell, no record excluded"""
    if dn == 'f64':
        assert R.high_ok()
    sym = S()
    for cls in range(4):
        assert n <= sym._chol_cap(TD[dn], cls)
    comp, vec, g, cells = C.batch(dn, n)
    assert C.judged(dn, n, comp).all(), 'no record of these cells may be excluded'
    m = C.truth(dn, n)
    x, v, gg = dev_of(comp, dev), dev_of(vec, dev), dev_of(g, dev)
    worst = {}
    for op in FORWARD_OPS:
        got = forward(op, x, v).cpu().numpy()
        assert np.isfinite(got).all(), op
        worst[op] = C.worst(C.forward_ratio(dn, m, op, got), cells)
    for op in C.SCALARS:
        val, packed = backward(op, x, v, gg)
        assert torch.equal(val, forward(op, x, v)), op
        packed = packed.cpu().numpy()
        assert np.isfinite(packed).all(), op
        worst[op + '_backward'] = C.worst(C.backward_ratio(dn, m, op, packed), cells)
    for op, w in worst.items():
        c = max(w, key=w.get)
        print(f'{dn} n={n} {op}: worst {w[c]:.3f} in {c} (of 1)')
    over = {op: w for op, w in worst.items() if max(w.values()) > 1.0}
    assert not over, over


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(dev, x):
    """{name: a tensor equal to x (nb, C) in another layout}"""
    nb, K = x.shape
    out = {}
    out['channel_first'] = x.t().contiguous().t()                                   # (K, nb) storage viewed as (nb, K)
    wide = torch.zeros(nb, K + 3, device=dev, dtype=x.dtype)
    wide[:, 1:K + 1] = x
    out['padded'] = wide[:, 1:K + 1]                                                 # a padded record stride
    flat = torch.zeros(nb * K + 1, device=dev, dtype=x.dtype)
    flat[1:] = x.reshape(-1)
    out['odd_offset'] = flat[1:].view(nb, K)                                         # base at an odd element offset
    return out


@pytest.mark.parametrize('n', [1, 3, 4, 6, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_layouts_give_the_same_bits(dev, dn, n):
    comp, vec, g, _ = C.batch(dn, n)
    x, v, gg = dev_of(comp, dev), dev_of(vec, dev), dev_of(g, dev)
    nb, K = x.shape
    ref = {op: forward(op, x, v) for op in FORWARD_OPS}
    gref = {op: backward(op, x, v, gg)[1] for op in C.SCALARS}
    xs, vs = _layouts(dev, x), _layouts(dev, v)
    for name in xs:
        for op in FORWARD_OPS:
            assert torch.equal(forward(op, xs[name], vs[name]), ref[op]), (name, op)
        for op in C.SCALARS:
            assert torch.equal(backward(op, xs[name], vs[name], gg)[1], gref[op]), (name, op)
    # a (3, 70) two-dimensional batch, as a slice of a larger field (two stride levels)
    big_x = torch.zeros(3, 80, K, device=dev, dtype=x.dtype)
    big_v = torch.zeros(3, 80, n, device=dev, dtype=x.dtype)
    big_x[:, :70] = x[:210].view(3, 70, K)
    big_v[:, :70] = v[:210].view(3, 70, n)
    for op in FORWARD_OPS:
        got = forward(op, big_x[:, :70], big_v[:, :70])
        assert got.shape[:2] == (3, 70) and torch.equal(got.reshape((210,) + got.shape[2:]), ref[op][:210]), op
    for op in C.SCALARS:
        got = backward(op, big_x[:, :70], big_v[:, :70], gg[:210].view(3, 70))[1]
        assert torch.equal(got.reshape(210, -1), gref[op][:210]), op
    # stride-0 operands: one matrix against 1200 vectors, one vector against 1200 matrices
    xb, vb = x[5:6].expand(nb, -1), v[7:8].expand(nb, -1)
    for op in C.APPLY + ('maha', 'maha_sqrt', 'logpdf'):
        assert torch.equal(forward(op, xb, v), forward(op, xb.contiguous(), v)), op
        assert torch.equal(forward(op, x[5], v), forward(op, xb.contiguous(), v)), op
        assert torch.equal(forward(op, x, vb), forward(op, x, vb.contiguous())), op
        assert torch.equal(forward(op, x, v[7]), forward(op, x, vb.contiguous())), op
    for op in ('maha', 'maha_sqrt', 'logpdf'):
        a = x[5].clone().requires_grad_(True)
        b = v.clone().requires_grad_(True)
        forward(op, a, b).backward(gg)
        full = backward(op, xb.contiguous(), v, gg)[1]
        assert a.grad.shape == (K,) and torch.equal(b.grad, full[:, K:]), op
        assert torch.equal(a.grad, full[:, :K].sum_to_size(K)), op
    # out= given: contiguous, and a slice of a wider tensor
    for op in FORWARD_OPS:
        out = torch.empty_like(ref[op])
        assert forward(op, x, v, out=out) is out and torch.equal(out, ref[op]), op
    wide = torch.zeros(nb, n + 2, device=dev, dtype=x.dtype)
    S().sym_chol_apply(x, v, 'Linv', out=wide[:, 1:n + 1])
    assert torch.equal(wide[:, 1:n + 1], ref['Linv']) and (wide[:, 0] == 0).all() and (wide[:, -1] == 0).all()
    inplace = x.clone()
    assert S().sym_chol(inplace, out=inplace) is inplace and torch.equal(inplace, ref['factor'])


# ------------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_ops_agree_with_each_other(dev, dn, n):
    sym = S()
    comp, vec, g, cells = C.batch(dn, n)
    x, v = dev_of(comp, dev), dev_of(vec, dev)
    m = C.truth(dn, n)
    hp = R.HP[dn]
    fac = sym.sym_chol(x)
    assert torch.equal(sym.sym_diag(fac), fac[:, :n]) and (fac[:, :n] > 0).all()
    for op in C.APPLY:
        assert torch.equal(sym.sym_chol_apply(fac, v, op, factored=True), sym.sym_chol_apply(x, v, op)), op
    b = C._bounds(dn, m)
    y = sym.sym_chol_apply(x, v, 'Linv').cpu().numpy().astype(hp)
    maha = sym.sym_mahalanobis(x, v).cpu().numpy().astype(hp)
    assert (np.abs(maha - (y * y).sum(-1)) <= b['maha']).all()
    logdet = sym.sym_logdet(x).cpu().numpy().astype(hp)
    logpdf = sym.sym_gauss_logpdf(x, v).cpu().numpy().astype(hp)
    assert (np.abs(logpdf + (n * hp(C.LOG_2PI) + logdet + maha) / 2) <= b['logpdf']).all()
    # the factor is scale equivariant bit for bit
    keep = np.ones(len(comp), bool)
    keep[cells['scaled']] = False
    s = 2.0 ** (20 if dn == 'f32' else 200)
    kx = x[torch.as_tensor(keep, device=dev)]
    assert torch.equal(sym.sym_chol(kx * (s * s)), sym.sym_chol(kx) * s)
    assert torch.equal(sym.sym_chol(kx / (s * s)), sym.sym_chol(kx) / s)


# ------------------------------------------------------------------------------------------------ bad records
@pytest.mark.parametrize('n', [1, 3, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_bad_records_are_nan_and_their_neighbours_untouched(dev, dn, n):
    comp, vec, g, _ = C.batch(dn, n)
    at = [0, 63, 64, 1199]
    mixed = np.array(comp)
    mixed[at] = C.bad_records(dn, n)
    good = torch.as_tensor(np.setdiff1d(np.arange(len(comp)), at), device=dev)
    x, xm, v, gg = dev_of(comp, dev), dev_of(mixed, dev), dev_of(vec, dev), dev_of(g, dev)
    for op in FORWARD_OPS:
        got, clean = forward(op, xm, v), forward(op, x, v)
        assert torch.isnan(got[at]).all(), op
        assert torch.equal(got[good], clean[good]), op
    for op in C.SCALARS:
        got, clean = backward(op, xm, v, gg)[1], backward(op, x, v, gg)[1]
        assert torch.isnan(got[at]).all(), op
        assert torch.equal(got[good], clean[good]), op
    # the differentiable factor (the torch composition) follows the same rule
    a = xm[:66].clone().requires_grad_(True)
    fac = S().sym_chol(a)
    fac.sum().backward()
    for r in (fac.detach(), a.grad):
        assert torch.isnan(r[[0, 63, 64]]).all() and torch.isfinite(r[1:63]).all()


def test_logdet_where_the_determinant_overflows(dev):
    sym = S()
    rng = np.random.default_rng(5)
    gm = rng.standard_normal((64, 8, 8))
    a = 1e6 * (gm @ gm.swapaxes(-1, -2) / 8 + np.eye(8))
    x = dev_of(R.pack(a).astype(np.float32), dev)
    logdet = sym.sym_logdet(x)
    assert torch.isfinite(logdet).all()
    assert torch.isinf(sym.sym_det(x).log()).all()
    want = np.linalg.slogdet(R.unpack(x.cpu().numpy().astype(np.float64), 8))[1]
    assert np.abs(logdet.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert torch.isfinite(sym.sym_logdet(x * 1e-12)).all()


@pytest.mark.parametrize('n', [1, 4, 8])
def test_root_gradient_at_zero_is_exactly_zero(dev, n):
    for dn in ('f32', 'f64'):
        comp, vec, g, _ = C.batch(dn, n)
        x, gg = dev_of(comp[:100], dev), dev_of(g[:100], dev)
        v = torch.zeros(100, n, device=dev, dtype=x.dtype)
        val, packed = backward('maha_sqrt', x, v, gg)
        assert (val == 0).all() and (packed == 0).all()


# ------------------------------------------------------------------------------------------------ caps and graphs
@pytest.mark.parametrize('n', [9, 12])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_orders_above_the_caps_take_the_composition(dev, dn, n):
    sym = S()
    for cls in range(4):
        assert n > sym._chol_cap(TD[dn], cls)
    rng = np.random.default_rng(900 + n)
    comp = R.pack(np.concatenate([C.cell(c, dn, rng, 16, n) for c in C.CELLS])).astype(R.NP[dn])
    vec = rng.standard_normal((len(comp), n)).astype(R.NP[dn])
    g = rng.standard_normal(len(comp)).astype(R.NP[dn])
    assert C.judged(dn, n, comp).all()
    m = C.model(dn, comp, vec, g)
    x, v, gg = dev_of(comp, dev), dev_of(vec, dev), dev_of(g, dev)
    for op in FORWARD_OPS:
        r = C.forward_ratio(dn, m, op, forward(op, x, v).cpu().numpy())
        assert r.max() <= 1.0, (op, float(r.max()))
    for op in C.SCALARS:
        r = C.backward_ratio(dn, m, op, backward(op, x, v, gg)[1].cpu().numpy())
        assert r.max() <= 1.0, (op, float(r.max()))
    bad = np.array(comp[:6])
    bad[1:5] = C.bad_records(dn, n)
    res = sym.sym_gauss_logpdf(dev_of(bad, dev), v[:6])
    assert torch.isnan(res[1:5]).all() and torch.isfinite(res[[0, 5]]).all()


def test_forward_and_backward_capture_in_a_graph(dev):
    """sym_gauss_logpdf, forward plus backward through autograd, captured in one graph on one stream and replayed twice
    on refreshed inputs: the bits of the eager call"""
    sym = S()
    n = 3
    comp, vec, g, _ = C.batch('f32', n)
    x = dev_of(comp, dev).requires_grad_(True)
    v = dev_of(vec, dev).requires_grad_(True)
    gg = dev_of(g, dev)

    def run(a, b):
        res = sym.sym_gauss_logpdf(a, b)
        res.backward(gg)
        return res

    def eager(a, b):
        a, b = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        res = run(a, b)
        return res.detach(), a.grad, b.grad

    side = torch.cuda.Stream(device=dev)         # warm-up outside the capture (module load, autograd's buffers)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(x, v)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    x.grad = v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run(x, v)
    for k in range(2):
        with torch.no_grad():
            x.mul_(1.25)
            v.mul_(-0.5)
            gg.mul_(2.0)
        graph.replay()
        torch.cuda.synchronize()
        re, ga, gb = eager(x, v)
        assert torch.equal(res.detach(), re) and torch.equal(x.grad, ga) and torch.equal(v.grad, gb), k


def test_empty_batch_and_dtype_argument(dev):
    sym = S()
    x = torch.empty(0, 6, device=dev)
    v = torch.empty(0, 3, device=dev)
    assert sym.sym_chol(x).shape == (0, 6) and sym.sym_chol_apply(x, v, 'L').shape == (0, 3)
    assert sym.sym_logdet(x).shape == (0,) and sym.sym_gauss_logpdf(x, v).shape == (0,)
    comp, vec, g, _ = C.batch('f32', 4)
    x32, v32 = dev_of(comp, dev), dev_of(vec, dev)
    r = sym.sym_gauss_logpdf(x32, v32, dtype=torch.float64)
    assert r.dtype == torch.float64 and torch.equal(r, sym.sym_gauss_logpdf(x32.double(), v32.double()))
    a = x32.clone().requires_grad_(True)
    sym.sym_mahalanobis(a, v32, dtype=torch.float64).sum().backward()
    assert a.grad.dtype == torch.float32 and torch.isfinite(a.grad).all()
