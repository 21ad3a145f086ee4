"""The backward kernels of the Cholesky factor on the GPU (the gradients of sym_chol and sym_chol_apply through
`.backward()`): every gradient on the whole batch of tests/_symchol_ref.py against the per-record bounds of
tests/_cholgrad_ref.py; the forward bits with and without requires_grad and the gradient's bits against the CPU entry;
every layout against the contiguous call bit for bit; what autograd saves; the bad-record rule; the consistency of the
direct gradient with the chain through sym_chol; graph capture; second derivatives; the composition above the caps; the
dtype argument and the empty batch."""
import numpy as np
import pytest
import torch
import _cholgrad_ref as G
import _symchol_ref as C
import _symfun_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'f64': torch.float64}
DT = {'f32': 0, 'f64': 1}
FACTOR, APPLY = 0, 1


def S():
    from nitorch_fastmath_amd import sym
    return sym


def dev_of(x, dev):
    return torch.as_tensor(np.array(x), device=dev)


def forward(op, mat, vec, factored=False, **kw):
    if op == 'factor':
        return S().sym_chol(mat, **kw)
    return S().sym_chol_apply(mat, vec, op, factored=factored, **kw)


def backward(op, mat, vec, cot, factored=False, **kw):
    """(value, packed gradient [K] of the factor or [K | n] of an apply op) through autograd"""
    a = mat.detach().requires_grad_(True)
    v = None if op == 'factor' else vec.detach().requires_grad_(True)
    res = forward(op, a, v, factored, **kw)
    res.backward(cot)
    return res.detach(), (a.grad if op == 'factor' else torch.cat([a.grad, v.grad], -1))


def host(dn, n, op, mat, vec, cot, factored=False):
    """`nfm_sym_chol_grad_host` on contiguous numpy records"""
    from nitorch_fastmath_amd import _lib
    T = R.NP[dn]
    mat, cot = np.ascontiguousarray(mat, T), np.ascontiguousarray(cot, T)
    vec = None if op == 'factor' else np.ascontiguousarray(vec, T)
    nb, K = mat.shape
    out = np.full((nb, K if op == 'factor' else K + n), 7.0, T)
    rc = _lib.lib().nfm_sym_chol_grad_host(DT[dn], n, C.CODE[op] | (C.FACTORED if factored else 0), nb, mat.ctypes.data,
                                           None if vec is None else vec.ctypes.data, cot.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out


def cases():
    """(op, factored) of every gradient the facade serves: with `factored` the gradient is with respect to the factor"""
    return [(op, False) for op in G.OPS] + [(op, True) for op in C.APPLY]


def inputs(dn, n, op, factored):
    comp, vec, _, cells = C.batch(dn, n)
    Gc, gc = G.cotangents(dn, n)
    return (G.factor_input(dn, n) if factored else comp), vec, (Gc if op == 'factor' else gc), cells


# ------------------------------------------------------------------------------------------------ the bounds, the bits
@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_every_gradient_meets_its_bounds(dev, dn, n):
    """the 1200 records through .backward(): every ratio <= 1 in every cell, no record excluded; the forward value has
    the bits of the call without requires_grad and the gradient the bits of the CPU entry (the same source; sqrt and
    the division are correctly rounded on both sides)"""
    if dn == 'f64':
        assert R.high_ok()
    sym = S()
    for cls in (FACTOR, APPLY):
        assert n <= sym._chol_grad_cap(TD[dn], cls)
    assert C.judged(dn, n, C.batch(dn, n)[0]).all(), 'no record of these cells may be excluded'
    worst = {}
    for op, factored in cases():
        mat, vec, cot, cells = inputs(dn, n, op, factored)
        x, v, g = dev_of(mat, dev), dev_of(vec, dev), dev_of(cot, dev)
        val, packed = backward(op, x, v, g, factored)
        assert torch.equal(val, forward(op, x, v, factored)), (op, factored)
        packed = packed.cpu().numpy()
        assert np.isfinite(packed).all(), (op, factored)
        r = G.ratio(dn, G.truth(dn, n, factored), op, packed, vec, cot)
        worst[op, factored] = C.worst(r, cells)
        assert np.array_equal(packed, host(dn, n, op, mat, vec, cot, factored)), (op, factored)
    for key, w in worst.items():
        c = max(w, key=w.get)
        print(f'{dn} n={n} {key}: worst {w[c]:.3f} in {c} (of 1)')
    over = {key: w for key, w in worst.items() if max(w.values()) > 1.0}
    assert not over, over


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(dev, x):
    """{name: a tensor equal to x (nb, C) in another layout}"""
    nb, K = x.shape
    out = {}
    out['channel_first'] = x.t().contiguous().t()                                   # (K, nb) storage viewed as (nb, K)
    wide = torch.zeros(nb, K + 3, device=dev, dtype=x.dtype)
    wide[:, 1:K + 1] = x
    out['padded'] = wide[:, 1:K + 1]                                                 # a slice of a wider field
    flat = torch.zeros(nb * K + 1, device=dev, dtype=x.dtype)
    flat[1:] = x.reshape(-1)
    out['odd_offset'] = flat[1:].view(nb, K)                                         # base at an odd element offset
    return out


@pytest.mark.parametrize('n', [1, 3, 4, 6, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_layouts_give_the_same_bits(dev, dn, n):
    comp, vec, _, _ = C.batch(dn, n)
    Gc, gc = G.cotangents(dn, n)
    x, v, gg, g = dev_of(comp, dev), dev_of(vec, dev), dev_of(Gc, dev), dev_of(gc, dev)
    nb, K = x.shape
    ref = {(op, f): backward(op, x, v, gg if op == 'factor' else g, f)[1] for op, f in cases()}
    xs, vs, ggs, gs = _layouts(dev, x), _layouts(dev, v), _layouts(dev, gg), _layouts(dev, g)
    for name in xs:
        for op, f in cases():
            got = backward(op, xs[name], vs[name], (ggs if op == 'factor' else gs)[name], f)[1]
            assert torch.equal(got, ref[op, f]), (name, op, f)
    # a (3, 70) two-dimensional batch, as a slice of a larger field (two stride levels)
    big_x = torch.zeros(3, 80, K, device=dev, dtype=x.dtype)
    big_v = torch.zeros(3, 80, n, device=dev, dtype=x.dtype)
    big_x[:, :70] = x[:210].view(3, 70, K)
    big_v[:, :70] = v[:210].view(3, 70, n)
    for op, f in cases():
        cot = (gg if op == 'factor' else g)[:210]
        got = backward(op, big_x[:, :70], big_v[:, :70], cot.view(3, 70, -1), f)[1]
        assert got.shape[:2] == (3, 70) and torch.equal(got.reshape(210, -1), ref[op, f][:210]), (op, f)
    # stride-0 operands: one matrix against 1200 vectors, one vector against 1200 matrices; the gradient of the
    # broadcast operand has the operand's own shape and is the sum of the per-record gradients
    xb, vb = x[5:6].expand(nb, -1).contiguous(), v[7:8].expand(nb, -1).contiguous()
    for op in C.APPLY:
        for f in (False, True):
            full = backward(op, xb, v, g, f)[1]
            for one in (x[5], x[5:6]):
                a, b = one.clone().requires_grad_(True), v.clone().requires_grad_(True)
                forward(op, a, b, f).backward(g)
                assert a.grad.shape == one.shape and torch.equal(b.grad, full[:, K:]), (op, f)
                assert torch.equal(a.grad, full[:, :K].sum_to_size(one.shape)), (op, f)
            full = backward(op, x, vb, g, f)[1]
            a, b = x.clone().requires_grad_(True), v[7].clone().requires_grad_(True)
            forward(op, a, b, f).backward(g)
            assert b.grad.shape == (n,) and torch.equal(a.grad, full[:, :K]), (op, f)
            assert torch.equal(b.grad, full[:, K:].sum_to_size(n)), (op, f)


# ------------------------------------------------------------------------------------------------ what is saved
@pytest.mark.parametrize('n', [3, 8])
def test_nothing_is_saved_but_inputs_and_output(dev, n):
    """under saved_tensors_hooks every tensor autograd keeps for sym_chol(a) and sym_chol_apply(a, v, op) shares its
    storage with an input or with the returned output (no full N x N matrix, no factor of its own)"""
    comp, vec, _, _ = C.batch('f32', n)
    for op, factored in cases():
        a = dev_of(comp, dev).requires_grad_(True)
        v = dev_of(vec, dev).requires_grad_(True)
        saved = []

        def pack(t):
            saved.append(t)
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            res = forward(op, a, v, factored)
        own = {t.untyped_storage().data_ptr() for t in (a, v, res)}
        assert saved, (op, factored)
        for t in saved:
            assert t.untyped_storage().data_ptr() in own, (op, factored, tuple(t.shape))


# ------------------------------------------------------------------------------------------------ bad records
@pytest.mark.parametrize('n', [1, 3, 8])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_bad_records_are_nan_and_their_neighbours_untouched(dev, dn, n):
    comp, vec, _, _ = C.batch(dn, n)
    Gc, gc = G.cotangents(dn, n)
    at = [0, 63, 64, 1199]
    mixed = np.array(comp)
    mixed[at] = C.bad_records(dn, n)
    good = torch.as_tensor(np.setdiff1d(np.arange(len(comp)), at), device=dev)
    x, xm, v = dev_of(comp, dev), dev_of(mixed, dev), dev_of(vec, dev)
    for op in G.OPS:
        cot = dev_of(Gc if op == 'factor' else gc, dev)
        (val, got), (cval, clean) = backward(op, xm, v, cot), backward(op, x, v, cot)
        assert torch.isnan(val[at]).all() and torch.isnan(got[at]).all(), op
        assert torch.equal(val[good], cval[good]) and torch.equal(got[good], clean[good]), op
        assert torch.isfinite(clean).all(), op
        # separately: a NaN in one cotangent (the value is what it was, both gradients of the record are NaN)
        nan_cot = cot.clone()
        nan_cot[777, -1] = float('nan')
        val, got = backward(op, x, v, nan_cot)
        rest = torch.arange(len(comp), device=dev) != 777
        assert torch.equal(val, cval) and torch.isnan(got[777]).all() and torch.equal(got[rest], clean[rest]), op
    # a factor that is not one, handed in as `factored`
    fac = np.array(G.factor_input(dn, n))
    fac[at[0], 0], fac[at[1], 0], fac[at[2], n - 1], fac[at[3], 0] = 0.0, -1.0, np.nan, np.inf
    f, fm, g = dev_of(G.factor_input(dn, n), dev), dev_of(fac, dev), dev_of(gc, dev)
    for op in C.APPLY:
        (val, got), (cval, clean) = backward(op, fm, v, g, True), backward(op, f, v, g, True)
        assert torch.isnan(val[at]).all() and torch.isnan(got[at]).all(), op
        assert torch.equal(val[good], cval[good]) and torch.equal(got[good], clean[good]), op


# ------------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize('n', C.ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_direct_gradient_agrees_with_the_chain_through_sym_chol(dev, dn, n):
    """the gradient of sym_chol_apply(a, v, op) against the gradient of sym_chol_apply(sym_chol(a), v, op,
    factored=True): both run the steps the bound of the direct gradient is derived for, so they differ by at most the
    sum of their bounds, twice that bound"""
    sym = S()
    comp, vec, _, cells = C.batch(dn, n)
    _, gc = G.cotangents(dn, n)
    x, v, g = dev_of(comp, dev), dev_of(vec, dev), dev_of(gc, dev)
    hp = R.HP[dn]
    K = comp.shape[-1]
    for op in C.APPLY:
        direct = backward(op, x, v, g)[1].cpu().numpy().astype(hp)
        a, b = x.clone().requires_grad_(True), v.clone().requires_grad_(True)
        res = sym.sym_chol_apply(sym.sym_chol(a), b, op, factored=True)
        assert torch.equal(res, sym.sym_chol_apply(x, v, op)), op
        res.backward(g)
        chain = torch.cat([a.grad, b.grad], -1).cpu().numpy().astype(hp)
        _, bS, _, bv = G.want(dn, G.truth(dn, n, False), op, vec, gc)
        rS = C._ratio(np.abs(R.unpack(direct[:, :K] - chain[:, :K], n, off=0.5)), 2 * bS)
        rv = C._ratio(np.abs(direct[:, K:] - chain[:, K:]), 2 * bv)
        assert max(rS.max(), rv.max()) <= 1.0, (op, C.worst(np.maximum(rS, rv), cells))


# ------------------------------------------------------------------------------------------------ graphs
def test_forward_and_backward_capture_in_a_graph(dev):
    """x = sym_chol_apply(a, eps, 'L') followed by x.square().sum().backward(), captured in one graph on one stream and
    replayed twice on refreshed inputs: the bits of the eager call"""
    sym = S()
    n = 3
    comp, vec, _, _ = C.batch('f32', n)
    a = dev_of(comp, dev).requires_grad_(True)
    e = dev_of(vec, dev).requires_grad_(True)

    def run(a, e):
        x = sym.sym_chol_apply(a, e, 'L')
        x.square().sum().backward()
        return x

    def eager(a, e):
        a, e = a.detach().clone().requires_grad_(True), e.detach().clone().requires_grad_(True)
        x = run(a, e)
        return x.detach(), a.grad, e.grad

    side = torch.cuda.Stream(device=dev)         # warm-up outside the capture (module load, autograd's buffers)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(a, e)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    a.grad = e.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x = run(a, e)
    for k in range(2):
        with torch.no_grad():
            a.mul_(1.25)
            e.mul_(-0.5)
        graph.replay()
        torch.cuda.synchronize()
        xe, ga, ge = eager(a, e)
        assert torch.equal(x.detach(), xe) and torch.equal(a.grad, ga) and torch.equal(e.grad, ge), k


# ------------------------------------------------------------------------------------------------ second derivatives
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_double_backward_takes_the_composition(dev, dn):
    """create_graph=True on 16 records of order 3: the second derivative is finite and is the composition's (both sides
    are the same torch ops, so this checks the routing)"""
    from nitorch_fastmath_amd import _symchol as Y
    sym = S()
    comp, vec, _, _ = C.batch(dn, 3)
    tol = 1e-4 if dn == 'f32' else 1e-10

    def second(f):
        a = dev_of(comp[:16], dev).requires_grad_(True)
        v = dev_of(vec[:16], dev).requires_grad_(True)
        res = f(a, v)
        ga, gv = torch.autograd.grad(res, (a, v), torch.ones_like(res), create_graph=True, allow_unused=True)
        assert ga.requires_grad
        loss = ga.square().sum() + (0 if gv is None else gv.square().sum())
        return torch.autograd.grad(loss, (a, v), allow_unused=True)

    pairs = [(lambda a, v: sym.sym_chol(a), lambda a, v: Y.chol(a))]
    for op in C.APPLY:
        pairs.append((lambda a, v, op=op: sym.sym_chol_apply(a, v, op), lambda a, v, op=op: Y.chol_apply(a, v, op)))
    pairs.append((lambda a, v: sym.sym_chol_apply(a, v, 'Linv', factored=True),
                  lambda a, v: Y.chol_apply(a, v, 'Linv', factored=True)))
    for ours, theirs in pairs:
        for got, want in zip(second(ours), second(theirs)):
            assert (got is None) == (want is None)
            if got is not None:
                assert torch.isfinite(got).all() and got.abs().max() > 0
                assert (got - want).abs().max() <= tol * want.abs().max()


# ------------------------------------------------------------------------------------------------ caps, dtype, empty
@pytest.mark.parametrize('n', [9, 12])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_orders_above_the_caps_take_the_composition(dev, dn, n):
    sym = S()
    for cls in (FACTOR, APPLY):
        assert n > sym._chol_grad_cap(TD[dn], cls)
    rng = np.random.default_rng(900 + n)
    comp = R.pack(np.concatenate([C.cell(c, dn, rng, 16, n) for c in C.CELLS])).astype(R.NP[dn])
    vec = rng.standard_normal((len(comp), n)).astype(R.NP[dn])
    Gc = rng.standard_normal(comp.shape).astype(R.NP[dn])
    gc = rng.standard_normal(vec.shape).astype(R.NP[dn])
    fac = G.pack_lower(C.chol_any(R.unpack(comp, n))).astype(R.NP[dn])
    judged = C.judged(dn, n, comp)
    for factored in (False, True):
        mat = fac if factored else comp
        m = G.model(dn, n, mat, factored)
        for op in (C.APPLY if factored else G.OPS):
            cot = Gc if op == 'factor' else gc
            packed = backward(op, dev_of(mat, dev), dev_of(vec, dev), dev_of(cot, dev), factored)[1].cpu().numpy()
            assert np.isfinite(packed).all(), (op, factored)
            r = G.ratio(dn, m, op, packed, vec, cot)
            assert r[judged].max(initial=0.0) <= 1.0, (op, factored, float(r[judged].max()))


def test_dtype_argument_and_empty_batch(dev):
    sym = S()
    comp, vec, _, _ = C.batch('f32', 4)
    Gc, gc = G.cotangents('f32', 4)
    x32, v32 = dev_of(comp, dev), dev_of(vec, dev)
    for op in G.OPS:
        cot = dev_of(Gc if op == 'factor' else gc, dev).double()
        a, v = x32.clone().requires_grad_(True), v32.clone().requires_grad_(True)
        res = forward(op, a, v, dtype=torch.float64)
        assert res.dtype == torch.float64 and torch.equal(res, forward(op, x32.double(), v32.double()))
        res.backward(cot)
        want = backward(op, x32.double(), v32.double(), cot)[1]
        K = comp.shape[-1]
        assert a.grad.dtype == torch.float32 and torch.equal(a.grad, want[:, :K].float())
        if op != 'factor':
            assert v.grad.dtype == torch.float32 and torch.equal(v.grad, want[:, K:].float())
    a = torch.empty(0, 6, device=dev, requires_grad=True)
    v = torch.empty(0, 3, device=dev, requires_grad=True)
    fac = sym.sym_chol(a)
    fac.sum().backward()
    assert fac.shape == (0, 6) and a.grad.shape == (0, 6)
    a.grad = None
    y = sym.sym_chol_apply(a, v, 'Linv')
    y.sum().backward()
    assert y.shape == (0, 3) and a.grad.shape == (0, 6) and v.grad.shape == (0, 3)
