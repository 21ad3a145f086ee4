"""GPU tests of `batched.batchsvdvals`, `batchsvd`, `batchpolar` and their gradients: the bounds of
tests/_polar_ref.py on every family (batches of NB records: two full tiles of the largest tile and a ragged tail), the
gradients against the mpmath fixture, bit-identity across layouts, bad and singular records in the middle of a tile,
the torch routes, graph capture, and `sym_logm` of the stretch."""
import functools
import numpy as np
import pytest
import torch
import _polar_ref as R

pytestmark = pytest.mark.gpu
CASES = [(dn, n) for dn in ('f32', 'f64') for n in R.ORDERS]
DEV = 'cuda:0'


def _B():
    from nitorch_fastmath_amd import batched
    return batched


def _gpu(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


def _same(x, y):
    """the same bits, NaN records (the gradient of a record of rank <= n - 2) in the same places"""
    return torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num())


@functools.lru_cache(maxsize=None)
def _input(dn, n):
    return _gpu(R.batch(dn, n)[0])


@functools.lru_cache(maxsize=None)
def _forward(dn, n):
    """the three contiguous calls, once per (dtype, order); read-only"""
    B, a = _B(), _input(dn, n)
    return B.batchsvdvals(a), B.batchsvd(a), B.batchpolar(a)


@functools.lru_cache(maxsize=None)
def _cotangents(dn, n):
    """cotangents for the whole batch: the fixture's on its records, standard normal on the rest"""
    gr, gp, gs = R.fixture_cotangents(dn, n)
    rng = np.random.default_rng(77 + n)
    m = R.NB - len(gr)
    full = lambda g, shape: _gpu(np.concatenate([g, rng.standard_normal((m,) + shape).astype(g.dtype)]))  # noqa: E731
    return full(gr, (n, n)), full(gp, (n, n)), full(gs, (n,))


def _polar_grad(a, gr, gp):
    x = a.detach().requires_grad_()
    Rr, P = _B().batchpolar(x)
    outs, gs = zip(*[(o, g) for o, g in ((Rr, gr), (P, gp)) if g is not None])
    return torch.autograd.grad(list(outs), x, list(gs))[0]


def _vals_grad(a, gs):
    x = a.detach().requires_grad_()
    return torch.autograd.grad(_B().batchsvdvals(x), x, gs)[0]


@functools.lru_cache(maxsize=None)
def _backward(dn, n):
    a = _input(dn, n)
    gr, gp, gs = _cotangents(dn, n)
    return _polar_grad(a, gr, None), _polar_grad(a, None, gp), _polar_grad(a, gr, gp), _vals_grad(a, gs)


# ------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize('dn,n', CASES)
def test_forward_bounds(dev, dn, n):
    S, svd, pol = _forward(dn, n)
    assert S.shape == (R.NB, n) and svd[0].shape == (R.NB, n, n) and pol[1].shape == (R.NB, n, n)
    ratios = R.forward_ratios(dn, n, _np(S), tuple(_np(x) for x in svd), tuple(_np(x) for x in pol))
    assert R.report(f'gpu {dn} {n}x{n}', ratios) <= 1.0


@pytest.mark.parametrize('dn,n', CASES)
def test_backward_bounds(dev, dn, n):
    nfix = R.NFIX * len(R.FAMILIES)
    g1, g2, g3, g4 = (_np(g) for g in _backward(dn, n))
    ratios = R.grad_ratios(dn, n, g1[:nfix], g2[:nfix], g3[:nfix], g4[:nfix])
    assert R.report(f'gpu gradient {dn} {n}x{n}', ratios) <= 1.0
    fam = R.batch(dn, n)[1]
    full = fam != R.FAMILIES.index('rankdef')
    for g in (g1, g2, g3, g4):
        assert np.isfinite(g[full]).all(), 'finite on every full-rank record, repeated and cluster included'


@pytest.mark.parametrize('dn,n', [(dn, n) for dn in ('f32', 'f64') for n in R.ORDERS if n > 1])
def test_torch_svd_gradient_fails_at_repeated_singular_values(dev, dn, n):
    """the README's claim: the gradient of `U @ Vh` through torch.linalg.svd is not finite, or outside the bound the
    backward kernel is held to, on the `repeated` family.  Fails loudly if that stops being true."""
    a, fam, gr, _, _, T, _, _ = R.grad_cases(dn, n)
    rep = fam == R.FAMILIES.index('repeated')
    x = _gpu(a[rep]).requires_grad_()
    U, _, Vh = torch.linalg.svd(x)
    (g,) = torch.autograd.grad(U @ Vh, x, _gpu(gr[rep]))
    g = _np(g)
    ref = R.torch_ref_polar_grad(a[rep], gr[rep], None)
    ratio = R.polar_grad_ratio(dn, g, T['gaR'][rep], ref, T['S'][rep], gr[rep], None)
    print(f'torch.linalg.svd gradient of U @ Vh, repeated {dn} {n}x{n}: ratio to the bound {ratio}')
    assert (ratio > 1.0).any()
    ours = R.polar_grad_ratio(dn, _np(_backward(dn, n)[0])[:len(a)][rep], T['gaR'][rep], ref, T['S'][rep], gr[rep], None)
    assert (ours <= 1.0).all()


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(a):
    """views with the values of `a` (NB, n, n) in other layouts"""
    nb, n = a.shape[0], a.shape[-1]
    out = {'channel-first': a.permute(1, 2, 0).contiguous().permute(2, 0, 1)}
    pad = torch.zeros(nb, n, n + 3, dtype=a.dtype, device=a.device)
    pad[..., :n] = a
    out['padded rows'] = pad[..., :n]
    rec = torch.zeros(nb, n * n + 5, dtype=a.dtype, device=a.device)
    rec[:, :n * n] = a.reshape(nb, -1)
    out['padded records'] = rec[:, :n * n].unflatten(-1, (n, n))
    flat = torch.zeros(a.numel() + 1, dtype=a.dtype, device=a.device)
    flat[1:] = a.reshape(-1)
    out['odd offset'] = flat[1:].view(nb, n, n)
    two = torch.zeros(2 * nb, n, n, dtype=a.dtype, device=a.device)
    two[::2] = a
    out['every other record'] = two[::2]
    return out


@pytest.mark.parametrize('dn,n', CASES)
def test_layouts_give_the_same_bits(dev, dn, n):
    B, a = _B(), _input(dn, n)
    S, svd, pol = _forward(dn, n)
    gr, gp, gs = _cotangents(dn, n)
    g1, g2, g3, g4 = _backward(dn, n)
    for name, v in _layouts(a).items():
        assert torch.equal(v, a), name
        assert torch.equal(B.batchsvdvals(v), S), name
        for x, y in zip(B.batchsvd(v), svd):
            assert torch.equal(x, y), name
        for x, y in zip(B.batchpolar(v), pol):
            assert torch.equal(x, y), name
        assert _same(_polar_grad(v, gr, gp), g3), name
        assert _same(_polar_grad(v, gr, None), g1), name
        assert _same(_vals_grad(v, gs), g4), name
    # cotangents in another layout
    lg = _layouts(gp)
    assert _same(_polar_grad(a, None, lg['channel-first']), g2)
    assert _same(_polar_grad(a, None, lg['padded rows']), g2)
    # a broadcast batch: one record for every lane
    one = a[5:6].expand(300, n, n)
    Rr, P = B.batchpolar(one)
    assert torch.equal(Rr, pol[0][5:6].expand(300, n, n)) and torch.equal(P, pol[1][5:6].expand(300, n, n))
    assert torch.equal(B.batchsvdvals(one), S[5:6].expand(300, n))
    assert _same(_polar_grad(one, gr[:300], gp[:300])[7], _polar_grad(a[5:6], gr[7:8], gp[7:8])[0])
    # side='left' is the right decomposition of the transposed view, transposed back
    Pl, Rl = B.batchpolar(a, side='left')[::-1]
    Rt, Pt = B.batchpolar(a.transpose(-1, -2))
    assert torch.equal(Rl, Rt.transpose(-1, -2)) and torch.equal(Pl, Pt)
    e = R.C * n * R.eps_of(dn)
    left = R._ratio(R.fro(_np(a) - R._mm(_np(Pl), _np(Rl))), e * R.fro(_np(a)))
    assert left.max() <= 1.0


def test_channel_first_is_handed_on(dev):
    B = _B()
    a = _input('f32', 3).permute(1, 2, 0).contiguous().permute(2, 0, 1)
    for x in B.batchsvd(a) + B.batchpolar(a) + (B.batchsvdvals(a),):
        assert x.stride(0) == 1, 'a channel-first operand gets channel-first results'


# ------------------------------------------------------------------------------------------------ bad and singular records
@pytest.mark.parametrize('dn,n', [(dn, n) for dn in ('f32', 'f64') for n in (2, 3, 8)])
def test_nan_and_singular_records_in_the_middle_of_a_tile(dev, dn, n):
    B, a = _B(), _input(dn, n)
    S, svd, pol = _forward(dn, n)
    gr, gp, gs = _cotangents(dn, n)
    g1, g2, g3, g4 = _backward(dn, n)
    b = a.clone()
    inan, izero, ione = 300, 301, 302
    b[inan, n - 1, 0] = float('nan')
    b[izero] = 0                                          # rank 0 <= n - 2
    b[ione] = b[ione, 0].clone().expand(n, n) if n > 2 else b[ione].clone()          # n > 2: rank 1 <= n - 2
    b[ione + 1, n - 1] = b[ione + 1, 0].clone()                   # rank n - 1: R is still differentiable
    keep = torch.ones(R.NB, dtype=torch.bool, device=a.device)
    keep[inan:ione + 2] = False
    S2, svd2, pol2 = B.batchsvdvals(b), B.batchsvd(b), B.batchpolar(b)
    for x, y in zip((S2,) + svd2 + pol2, (S,) + svd + pol):
        assert torch.equal(x[keep], y[keep]), 'the neighbours do not notice'
        assert torch.isnan(x[inan]).all(), 'the NaN record is NaN throughout'
        assert torch.isfinite(x[izero:ione + 2]).all()
    sing = _np(b[izero:ione + 2])
    ratios = R.svd_ratios(dn, sing, *(_np(x[izero:ione + 2]) for x in svd2))
    pr, sym = R.polar_self_ratios(dn, sing, _np(pol2[0][izero:ione + 2]), _np(pol2[1][izero:ione + 2]),
                                  np.linalg.svd(sing.astype(np.float64), compute_uv=False)[:, 0])
    ratios.update(pr)
    assert sym and R.report(f'singular records {dn} {n}x{n}', ratios) <= 1.0
    assert float(S2[izero].abs().max()) == 0.0
    h1, h2, h3 = _polar_grad(b, gr, None), _polar_grad(b, None, gp), _polar_grad(b, gr, gp)
    h4 = _vals_grad(b, gs)
    for h, g, with_gr in ((h1, g1, True), (h2, g2, False), (h3, g3, True), (h4, g4, False)):
        assert _same(h[keep], g[keep])
        assert torch.isnan(h[inan]).all()
        assert torch.isfinite(h[ione + 1]).all(), 'rank n - 1: finite'
        if with_gr:
            assert torch.isnan(h[izero]).all(), 'rank <= n - 2 with a non-zero gR: NaN'
            assert torch.isnan(h[ione]).all() == (n > 2)
        else:
            assert torch.isfinite(h[izero]).all() and torch.isfinite(h[ione]).all()


# ------------------------------------------------------------------------------------------------ the torch routes
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_orders_above_the_cap_take_the_torch_route(dev, dn):
    from nitorch_fastmath_amd import _lib
    B = _B()
    for code, name in ((R.VALS, 'svdvals'), (R.FULL, 'svd'), (R.POLAR, 'polar'), (R.BWD, 'polar_backward')):
        assert B.polar_max_order(R.TT[dn], name) == _lib.lib().nfm_polar_max_order(R.CODE[dn], code)
    n = 9
    a = np.random.default_rng(9).standard_normal((200, n, n)).astype(R.NP[dn])
    a[3, 2, 2] = np.nan
    ok = np.arange(200) != 3
    x = _gpu(a)
    S = _np(B.batchsvdvals(x))
    U, S2, Vh = (_np(t) for t in B.batchsvd(x))
    Rr, P = (_np(t) for t in B.batchpolar(x))
    for t in (S, U, S2, Vh, Rr, P):
        assert np.isnan(t[3]).all() and np.isfinite(t[ok]).all()
    St = np.linalg.svd(a[ok].astype(np.float64), compute_uv=False)
    ratios = R.svd_ratios(dn, a[ok], U[ok], S2[ok], Vh[ok])
    pr, sym = R.polar_self_ratios(dn, a[ok], Rr[ok], P[ok], St[:, 0])
    ratios.update(pr)
    if dn == 'f32':
        ratios['values'] = R.vals_ratio(dn, S[ok], St)
    assert sym and R.ordered(S[ok]) and R.report(f'torch route {dn} {n}x{n}', ratios) <= 1.0
    g = _polar_grad(x, torch.ones_like(x), torch.ones_like(x))
    assert torch.isfinite(g[torch.from_numpy(ok).to(DEV)]).all() and torch.isnan(g[3]).all()


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_batchsvd_with_a_gradient_is_torch_linalg_svd(dev, dn):
    a, fam = R.batch(dn, 4)
    sel = fam == R.FAMILIES.index('normal')
    x = _gpu(a[sel]).requires_grad_()
    U, S, Vh = _B().batchsvd(x)
    assert 'Svd' in type(S.grad_fn).__name__
    ratios = R.svd_ratios(dn, a[sel], _np(U), _np(S), _np(Vh))
    if dn == 'f32':
        ratios['values'] = R.vals_ratio(dn, _np(S), R.truth64(a[sel])[0])
    assert R.report(f'batchsvd with grad {dn}', ratios) <= 1.0
    (g,) = torch.autograd.grad(S.sum(), x)
    assert torch.isfinite(g).all()


# ------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize('dn,n', [('f32', 3), ('f64', 4)])
def test_graph_capture_replays_the_eager_bits(dev, dn, n):
    B, a = _B(), _input(dn, n)
    S, svd, pol = _forward(dn, n)
    gr, gp, _ = _cotangents(dn, n)
    g3 = _backward(dn, n)[2]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up off the capturing stream
        B.batchsvdvals(a), B.batchsvd(a), B.batchpolar(a), B._polar_backward(a, gr, gp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = (B.batchsvdvals(a),) + tuple(B.batchsvd(a)) + tuple(B.batchpolar(a)) + (B._polar_backward(a, gr, gp),)
    for x in c:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(c, (S,) + svd + pol + (g3,)):
        assert _same(x, y)


# ------------------------------------------------------------------------------------------------ with sym_funm
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_sym_logm_of_the_stretch(dev, dn):
    """Hencky strain: sym_logm of the compact pack of P, end to end.  |Y^ - Y| <= C n eps ((1 + sqrt 2) s_1 / s_n + |Y|_2):
    P's own bound through the Lipschitz constant 1 / s_n of the logarithm, plus sym_funm's forward bound."""
    from nitorch_fastmath_amd import sym
    n = 3
    a, fam = R.batch(dn, n)
    sel = fam == R.FAMILIES.index('normal')
    x = _gpu(a[sel])
    P = _B().batchpolar(x)[1]
    comp = torch.cat([P.diagonal(dim1=-2, dim2=-1)] + [P[:, i, i + 1:] for i in range(n - 1)], -1)
    Y = _np(sym.sym_to_full(sym.sym_logm(comp)))
    _, s, vh = np.linalg.svd(a[sel].astype(np.float64))
    Yt = np.swapaxes(vh, -1, -2) @ (np.log(s)[:, :, None] * vh)
    bound = R.C * n * R.eps_of(dn) * ((1 + np.sqrt(2.0)) * s[:, 0] / s[:, -1] + np.abs(np.log(s)).max(-1))
    ratio = R._ratio(R.fro(Y - Yt), bound)
    print(f'sym_logm(P) {dn}: worst ratio {ratio.max():.3g}')
    assert ratio.max() <= 1.0
