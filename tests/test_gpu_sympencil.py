"""The two-matrix spectral functions of `sym` on the GPU (`sym_pencil_funm` and its wrappers, `sym_geneigvals`,
`sym_dist`, `sym_karcher_mean`): per-record conditioning bounds of the results and of the gradients against the model
of tests/_sympencil_ref.py (the constant C and where it comes from: that module's docstring), the identities between
the functions, every layout against the contiguous call bit for bit, the NaN-record rule, the composition route above
the compiled caps, graph capture, and the Karcher mean."""
import numpy as np
import pytest
import torch
import _symfun_ref as R
import _sympencil_ref as P

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'f64': torch.float64}
ORDERS = (1, 2, 3, 4, 6, 7, 8)          # 7: the float64 caps of the function and of the distance gradients
FUNM, FUNM_BWD, EIG, DIST_BWD = range(4)
POWERS = {'pow': P.POW_P, 'sqrt': 0.5, 'rsqrt': -0.5}


def S():
    from nitorch_fastmath_amd import sym
    return sym


def cap(dn, op):
    return S()._pencil_cap(TD[dn], op)


def T(dev, x, grad=False):
    return torch.as_tensor(np.array(x), device=dev).requires_grad_(grad)


def report(tag, cells, ratio):
    for fam, sl in cells.items():
        print(f'{tag} {fam}: {np.nanmax(ratio[sl]):.2f} (of {P.C})')


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize('fn', P.FUNCS)
@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_function_and_gradient_bounds(dev, dn, n, fn):
    """per record, every family: the result and the gradient with respect to `mat` within C of their bounds and
    finite; for the powers the gradient with respect to `base` against the model of the swapped pencil
    (A #_t B = B #_(1-t) A), its bound taken on the pair at unit scale (`grad_ratio`: with the bound as stated,
    2709 records reach 35.09 of 32 for rsqrt, float32, n = 3, B = s A, where ||B|| is up to 20 and the stated bound is
    below the rounding of the gradient itself).  Orders above a cap take the composition, held to the same bounds."""
    if dn == 'f64':
        assert R.high_ok()
    per = P.per_gpu(dn, n)
    ca, cb, cells = P.batch(dn, n, fn, per)
    g = P.cotangent(dn, n, len(ca))
    mod = P.truth(dn, n, fn, per)
    a, b = T(dev, ca, fn in POWERS), T(dev, cb, True)
    y = S().sym_pencil_funm(a, b, fn, p=P.fn_p(fn))
    y.backward(T(dev, g))
    y, gb = y.detach().cpu().numpy(), b.grad.cpu().numpy()
    assert np.isfinite(y).all() and np.isfinite(gb).all()
    rf, rb = P.fun_ratio(dn, fn, mod, y), P.grad_ratio(dn, fn, mod, g, gb)
    report(f'{fn} {dn} n={n} forward', cells, rf)
    report(f'{fn} {dn} n={n} gradient(mat)', cells, rb)
    assert rf.max() <= P.C, (rf.max(), int(rf.argmax()))
    assert rb.max() <= P.C, (rb.max(), int(rb.argmax()))
    if fn in POWERS:
        ga = a.grad.cpu().numpy()
        assert np.isfinite(ga).all()
        swapped = P.model(dn, 'pow', cb, ca, 1.0 - POWERS[fn], g)
        ra = P.grad_ratio(dn, 'pow', swapped, g, ga, unit_scale=True)
        report(f'{fn} {dn} n={n} gradient(base)', cells, ra)
        assert ra.max() <= P.C, (ra.max(), int(ra.argmax()))


@pytest.mark.parametrize('fn', ['log', 'exp'])
def test_base_gradient_of_log_and_exp_is_the_compositions(dev, fn):
    """with respect to `base`, log and exp take autograd through the composition: finite on every family, and the
    value autograd gives for the composition itself"""
    from nitorch_fastmath_amd import _sympencil
    ca, cb, _ = P.batch('f64', 3, fn)
    g = T(dev, P.cotangent('f64', 3, len(ca)))
    a = T(dev, ca, True)
    S().sym_pencil_funm(a, T(dev, cb), fn).backward(g)
    assert torch.isfinite(a.grad).all()
    a2 = T(dev, ca, True)
    _sympencil.pencil_funm(a2, T(dev, cb), R.FUNCS.index(fn)).backward(g)
    assert torch.equal(a.grad, a2.grad)


@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_eigenvalue_and_distance_bounds(dev, dn, n):
    if dn == 'f64':
        assert R.high_ok()
    sym = S()
    eps = R.eps_of(dn)
    per = P.per_gpu(dn, n)
    ca, cb, cells = P.batch(dn, n, 'log', per)
    mod = P.truth(dn, n, 'log', per)
    a, b = T(dev, ca, True), T(dev, cb, True)
    mu = sym.sym_geneigvals(b.detach(), a.detach()).cpu().numpy()
    assert np.isfinite(mu).all() and (np.diff(mu, axis=1) >= 0).all()
    re = P.eig_ratio(dn, mod, mu)
    report(f'{dn} n={n} eigenvalues', cells, re)
    assert re.max() <= P.C, (re.max(), int(re.argmax()))
    d2 = sym.sym_dist(a, b, squared=True)
    d2.sum().backward()
    ga, gb, d2 = a.grad.cpu().numpy(), b.grad.cpu().numpy(), d2.detach().cpu().numpy()
    assert np.isfinite(d2).all() and np.isfinite(ga).all() and np.isfinite(gb).all()
    rd = P.dist2_ratio(dn, mod, d2)
    ra, rb = P.dist_grad_ratios(dn, mod, ga, gb)
    for tag, r in (('d2', rd), ('d2 gradient(a)', ra), ('d2 gradient(b)', rb)):
        report(f'{dn} n={n} {tag}', cells, r)
        assert r.max() <= P.C, (tag, r.max(), int(r.argmax()))
    worst = max(np.abs(ga[cells['equal']]).max(), np.abs(gb[cells['equal']]).max())
    print(f'{dn} n={n} gradients of d2 at a = b: {worst / (n * eps):.2f} n eps (of {P.C})')
    assert worst <= P.C * n * eps
    # the distance itself: |d^ - d| = |d^2 - d2| / (d^ + d) <= min(|.| / d, sqrt |.|), and the rounding of the root
    d = sym.sym_dist(a.detach(), b.detach()).cpu().numpy().astype(np.float64)
    want = np.sqrt(mod['d2'].astype(np.float64))
    bound = P.C * P.dist2_bound(dn, mod)
    with np.errstate(divide='ignore'):
        assert (np.abs(d - want) <= np.minimum(bound / want, np.sqrt(bound)) + 2 * eps * want).all()
    # its gradients are finite at a = b and b = s a (defined as 0 at d = 0)
    a.grad = b.grad = None
    sym.sym_dist(a, b).sum().backward()
    for fam in ('equal', 'multiple'):
        assert torch.isfinite(a.grad[cells[fam]]).all() and torch.isfinite(b.grad[cells[fam]]).all()


# ------------------------------------------------------------------------------------------------ identities
def _err(dn, n, x, y):
    hp = R.HP[dn]
    return R._fro(R.unpack(np.asarray(x).astype(hp), n) - R.unpack(np.asarray(y).astype(hp), n))


@pytest.mark.parametrize('n', [3, 6])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_identities(dev, dn, n):
    """each within the sum of the two sides' bounds (C times the model's forward bounds)"""
    sym = S()
    eps = R.eps_of(dn)
    ca, cb, cells = P.batch(dn, n, 'pow')
    a, b = T(dev, ca), T(dev, cb)
    num = lambda t: t.cpu().numpy()          # noqa: E731
    t = P.POW_P
    left, right = P.truth(dn, n, 'pow'), P.model(dn, 'pow', cb, ca, 1 - t)
    err = _err(dn, n, num(sym.sym_geodesic(a, b, t)), num(sym.sym_geodesic(b, a, 1 - t)))
    assert (err <= P.C * (P.fun_bound(dn, 'pow', left) + P.fun_bound(dn, 'pow', right))).all()
    for tt, want in ((0.0, ca), (1.0, cb)):
        m = P.model(dn, 'pow', ca, cb, tt)
        assert (_err(dn, n, num(sym.sym_geodesic(a, b, tt)), want) <= P.C * P.fun_bound(dn, 'pow', m)).all(), tt
    m = P.model(dn, 'sqrt', ca, cb)
    assert (_err(dn, n, num(sym.sym_geomean(a, b)), num(sym.sym_geodesic(a, b, 0.5)))
            <= 2 * P.C * P.fun_bound(dn, 'sqrt', m)).all()
    # expmap(a, logmap(a, b)) = b: the error of the logarithm goes through exp with its Lipschitz constant L
    lg = sym.sym_logmap(a, b)
    ml, me = P.model(dn, 'log', ca, cb), P.model(dn, 'exp', ca, num(lg))
    bound = P.C * (P.fun_bound(dn, 'log', ml) * me['L'] * me['kappa'] + P.fun_bound(dn, 'exp', me))
    assert (_err(dn, n, num(sym.sym_expmap(a, lg)), cb) <= bound).all()
    # the distance is symmetric, and it is the norm of the logarithm of the whitened matrix
    dab, dba = num(sym.sym_dist(a, b, squared=True)), num(sym.sym_dist(b, a, squared=True))
    mab, mba = P.model(dn, 'log', ca, cb), P.model(dn, 'log', cb, ca)
    assert (np.abs(dab - dba) <= P.C * (P.dist2_bound(dn, mab) + P.dist2_bound(dn, mba))).all()
    r = sym.sym_to_full(sym.sym_rsqrtm(a))
    lc = sym.sym_to_full(sym.sym_logm(sym.sym_matmul(r, b)))
    viaC = num((lc * lc).sum((-1, -2)))
    slack = P.C * n * eps * (1 + mab['d2'].astype(np.float64))
    assert (np.abs(dab - viaC) <= 2 * P.C * P.dist2_bound(dn, mab) + slack).all()
    # base = I: the single-matrix function
    eye = torch.zeros(b.shape[-1], device=dev, dtype=b.dtype)
    eye[:n] = 1
    for fn in ('log', 'sqrt'):
        m = R.model(dn, fn, cb)
        bound = 2 * R.C * n * eps * (m['L'] * m['normA'] + m['normY'])
        assert (_err(dn, n, num(sym.sym_pencil_funm(eye, b, fn)), num(sym.sym_funm(b, fn))) <= bound).all(), fn


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(dev, x):
    """{name: a tensor equal to x in another layout} (the construction of tests/test_gpu_symfun.py)"""
    nb, K = x.shape
    out = {}
    out['channel_first'] = x.t().contiguous().t()
    wide = torch.zeros(nb, K + 3, device=dev, dtype=x.dtype)
    wide[:, 1:K + 1] = x
    out['padded'] = wide[:, 1:K + 1]
    flat = torch.zeros(nb * K + 1, device=dev, dtype=x.dtype)
    flat[1:] = x.reshape(-1)
    out['odd_offset'] = flat[1:].view(nb, K)
    return out


@pytest.mark.parametrize('n', [3, 6])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_layouts_give_the_same_bits(dev, dn, n):
    sym = S()
    ca, cb, _ = P.batch(dn, n, 'log')
    a, b, g = T(dev, ca), T(dev, cb), T(dev, P.cotangent(dn, n, len(ca)))
    bwd_kernel = n <= cap(dn, FUNM_BWD)
    dist_kernel = n <= cap(dn, DIST_BWD)

    def both(aa, bb, gg):
        aa, bb = aa.detach().requires_grad_(True), bb.detach().requires_grad_(True)
        y = sym.sym_geodesic(aa, bb, 0.3)
        y.backward(gg)
        ad = aa.detach().requires_grad_(True)
        d = sym.sym_dist(ad, bb, squared=True)
        da, db = torch.autograd.grad(d, (ad, bb), gg[:, 0])          # a strided one-value cotangent
        return y.detach(), aa.grad, bb.grad, d.detach(), db, da

    ref = both(a, b, g)
    la, lb, lg = _layouts(dev, a), _layouts(dev, b), _layouts(dev, g)
    for name in la:
        got = both(la[name], lb[name], lg[name])
        assert torch.equal(got[0], ref[0]) and torch.equal(got[3], ref[3]), name
        if bwd_kernel:
            assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), name
        if dist_kernel:
            assert torch.equal(got[4], ref[4]) and torch.equal(got[5], ref[5]), name
        plain = sym.sym_logmap(la[name], lb[name])
        assert torch.equal(plain, sym.sym_logmap(a, b)), name
        assert torch.equal(sym.sym_geneigvals(lb[name], la[name]), sym.sym_geneigvals(b, a)), name
        if name == 'channel_first':          # the layout is handed on
            assert plain.stride() == lb[name].stride() and got[0].stride() == lb[name].stride()
        # one operand in the other layout only
        assert torch.equal(sym.sym_logmap(la[name], b), sym.sym_logmap(a, b)), name
        assert torch.equal(sym.sym_logmap(a, lb[name]), sym.sym_logmap(a, b)), name
    # a stride-0 base against a batch of mat, and the reverse
    y0 = sym.sym_logmap(a[5:6].expand(len(b), -1).contiguous(), b)
    assert torch.equal(sym.sym_logmap(a[5], b), y0) and torch.equal(sym.sym_logmap(a[5:6].expand(len(b), -1), b), y0)
    assert torch.equal(sym.sym_dist(a, b[7]), sym.sym_dist(a, b[7:8].expand(len(a), -1).contiguous()))
    if bwd_kernel:          # the gradient of a broadcast base is summed over the batch
        ar = a[5].clone().requires_grad_(True)
        sym.sym_geodesic(ar, b[:64], 0.3).backward(g[:64])
        ac = a[5:6].expand(64, -1).contiguous().requires_grad_(True)
        sym.sym_geodesic(ac, b[:64], 0.3).backward(g[:64])
        assert ar.grad.shape == ar.shape and torch.equal(ar.grad, ac.grad.sum(0))
    if dist_kernel:          # the distance's cotangent contiguous, at stride 2, and broadcast at stride 0
        def dgrads(g1):
            ad, bd = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
            return torch.autograd.grad(sym.sym_dist(ad, bd, squared=True), (ad, bd), g1)
        g1 = g[:, 0].contiguous()
        two = torch.zeros(2 * len(g1), device=dev, dtype=g1.dtype)
        two[::2] = g1
        for x, y in zip(dgrads(g1), dgrads(two[::2])):
            assert torch.equal(x, y)
        for x, y in zip(dgrads(g1[3].expand(len(g1))), dgrads(g1[3].expand(len(g1)).contiguous())):
            assert torch.equal(x, y)
    # out= given, out=mat and out=base (in place)
    y0 = sym.sym_logmap(a, b)
    out = torch.empty_like(b)
    assert sym.sym_logmap(a, b, out=out) is out and torch.equal(out, y0)
    bi = b.clone()
    assert sym.sym_logmap(a, bi, out=bi) is bi and torch.equal(bi, y0)
    ai = a.clone()
    assert sym.sym_logmap(ai, b, out=ai) is ai and torch.equal(ai, y0)


@pytest.mark.parametrize('squared', [True, False])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_distance_gradient_of_a_broadcast_operand(dev, dn, squared):
    """one reference matrix against a field (stride 0, a size-1 dim, and no batch dim at all): its gradient is the sum
    of the gradients of the materialised batch, at the kernel's cap and one order above it (the composition)"""
    sym = S()
    eps = R.eps_of(dn)
    for n in (3, cap(dn, DIST_BWD), cap(dn, DIST_BWD) + 1):
        ca, cb, cells = P.batch(dn, n, 'log')
        sl = cells['normal']
        a, b, g1 = T(dev, ca[sl]), T(dev, cb[sl]), T(dev, P.cotangent(dn, n, len(ca))[sl, 0])
        full_a = a[5:6].expand(len(b), -1).contiguous().requires_grad_(True)
        bm = b.clone().requires_grad_(True)
        sym.sym_dist(full_a, bm, squared=squared).backward(g1)
        want, want_b = full_a.grad.sum(0), bm.grad
        tol = 64 * eps * len(b) * float(full_a.grad.abs().max())          # the order of the sum
        for shape in ('no batch dim', 'size-1 dim', 'stride 0'):
            ar = (a[5] if shape == 'no batch dim' else a[5:6]).clone().requires_grad_(True)
            br = b.clone().requires_grad_(True)
            view = ar.expand(len(b), -1) if shape == 'stride 0' else ar
            sym.sym_dist(view, br, squared=squared).backward(g1)
            assert ar.grad.shape == ar.shape
            assert float((ar.grad.reshape(-1) - want).abs().max()) <= tol, (n, shape)
            assert float((br.grad - want_b).abs().max()) <= 64 * eps * float(want_b.abs().max()), (n, shape)
        # and the broadcast second operand
        full_b = b[7:8].expand(len(a), -1).contiguous().requires_grad_(True)
        sym.sym_dist(a, full_b, squared=squared).backward(g1)
        br = b[7].clone().requires_grad_(True)
        sym.sym_dist(a, br, squared=squared).backward(g1)
        assert float((br.grad - full_b.grad.sum(0)).abs().max()) <= tol, n


# ------------------------------------------------------------------------------------------------ NaN records
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_bad_records_are_nan_and_their_neighbours_untouched(dev, dn):
    sym = S()
    n = 3
    ca, cb, _ = P.batch(dn, n, 'log')
    g = T(dev, P.cotangent(dn, n, len(ca)))

    def run(xa, xb):
        a, b = T(dev, xa, True), T(dev, xb, True)
        y = sym.sym_geodesic(a, b, 0.3)
        y.backward(g)
        d = sym.sym_dist(a.detach().requires_grad_(True), b.detach().requires_grad_(True), squared=True)
        res = [y.detach(), a.grad, b.grad, sym.sym_logmap(a.detach(), b.detach()),
               sym.sym_geneigvals(b.detach(), a.detach()), d.detach()]
        return [r.cpu().numpy().reshape(len(xa), -1) for r in res]

    clean = run(ca, cb)
    xa, xb = np.array(ca), np.array(cb)
    neg, nan_a, nan_b, neg_b = 100, 171, 30, 260          # between good records
    xa[neg] = R.pack(-np.diag([1.0, 0.5, 2.0])[None])[0]          # a negative definite base
    xa[nan_a, 4] = np.nan
    xb[nan_b, 0] = np.inf
    xb[neg_b] = R.pack(np.diag([1.0, -0.5, 2.0])[None])[0]          # mu < 0: outside the domain of pow and log
    bad = run(xa, xb)
    others = np.ones(len(ca), bool)
    others[[neg, nan_a, nan_b, neg_b]] = False
    for k, (r, r0) in enumerate(zip(bad, clean)):
        assert np.isnan(r[[neg, nan_a, nan_b]]).all(), k
        assert np.array_equal(r[others], r0[others]), k
        if k != 4:          # the eigenvalues of an indefinite mat are fine; every function of them is not
            assert np.isnan(r[neg_b]).all(), k
    assert np.isfinite(bad[4][neg_b]).all() and bad[4][neg_b].min() < 0


# ------------------------------------------------------------------------------------------------ the composition route
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_orders_above_the_caps(dev, dn):
    """one order above the forward cap the facade runs the composition and meets the bounds; one order below it the
    composition agrees with the kernel within the sum of the bounds"""
    from nitorch_fastmath_amd import _sympencil
    sym = S()
    n = cap(dn, FUNM) + 1
    for fn in ('log', 'pow'):
        ca, cb, _ = P.batch(dn, n, fn)
        g = P.cotangent(dn, n, len(ca))
        mod = P.truth(dn, n, fn)
        b = T(dev, cb, True)
        y = sym.sym_pencil_funm(T(dev, ca), b, fn, p=P.fn_p(fn))
        y.backward(T(dev, g))
        rf = P.fun_ratio(dn, fn, mod, y.detach().cpu().numpy())
        rb = P.grad_ratio(dn, fn, mod, g, b.grad.cpu().numpy())
        print(f'{fn} {dn} n={n}: forward {rf.max():.2f} gradient {rb.max():.2f} (of {P.C})')
        assert rf.max() <= P.C and rb.max() <= P.C
    ca, cb, _ = P.batch(dn, n, 'log')
    mod = P.truth(dn, n, 'log')
    assert P.eig_ratio(dn, mod, sym.sym_geneigvals(T(dev, cb), T(dev, ca)).cpu().numpy()).max() <= P.C
    assert P.dist2_ratio(dn, mod, sym.sym_dist(T(dev, ca), T(dev, cb), squared=True).cpu().numpy()).max() <= P.C
    out = torch.empty(len(ca), ca.shape[1], device=dev, dtype=TD[dn])
    assert sym.sym_logmap(T(dev, ca), T(dev, cb), out=out) is out
    n = cap(dn, FUNM) - 1
    ca, cb, _ = P.batch(dn, n, 'log')
    mod = P.model(dn, 'log', ca, cb)
    kern = sym.sym_logmap(T(dev, ca), T(dev, cb)).cpu().numpy()
    comp = _sympencil.pencil_funm(T(dev, ca), T(dev, cb), 1).cpu().numpy()
    assert (_err(dn, n, kern, comp) <= 2 * P.C * P.fun_bound(dn, 'log', mod)).all()


# ------------------------------------------------------------------------------------------------ graphs
def test_forward_and_backward_capture_in_a_graph(dev):
    """function and distance, forward plus backward, captured in one graph and replayed on refreshed inputs: the bits
    of the eager call"""
    sym = S()
    n = 3
    ca, cb, _ = P.batch('f32', n, 'pow')
    a, b = T(dev, ca, True), T(dev, cb, True)
    g = T(dev, P.cotangent('f32', n, len(ca)))

    def work(aa, bb, gg):
        y = sym.sym_geodesic(aa, bb, 0.3)
        d = sym.sym_dist(aa, bb, squared=True)
        torch.autograd.backward([y, d], [gg, gg[:, 0]])
        return y, d

    def eager(aa, bb, gg):
        aa, bb = aa.detach().clone().requires_grad_(True), bb.detach().clone().requires_grad_(True)
        y, d = work(aa, bb, gg)
        return y.detach(), d.detach(), aa.grad, bb.grad

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work(a, b, g)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    a.grad = b.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, d = work(a, b, g)
    for k in range(2):
        with torch.no_grad():
            a.mul_(1.25)
            g.mul_(-0.5)
        graph.replay()
        torch.cuda.synchronize()
        ye, de, ga, gb = eager(a, b, g)
        assert torch.equal(y.detach(), ye) and torch.equal(d.detach(), de), k
        assert torch.equal(a.grad, ga) and torch.equal(b.grad, gb), k


# ------------------------------------------------------------------------------------------------ the Karcher mean
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_karcher_mean(dev, dn):
    sym = S()
    n, eps = 3, R.eps_of(dn)
    rng = np.random.default_rng(5)
    num = lambda t: t.cpu().numpy()          # noqa: E731
    # a commuting set: the log-Euclidean mean
    q = R._orth(rng, 256, n)
    sets = np.stack([np.einsum('bij,bj,bkj->bik', q, rng.uniform(0.5, 4.0, (256, n)), q) for _ in range(5)])
    x = T(dev, R.pack(P._sym(sets)).astype(R.NP[dn]))          # (5, 256, K)
    w = torch.tensor([0.1, 0.2, 0.3, 0.25, 0.15], device=dev, dtype=TD[dn])
    got = sym.sym_karcher_mean(x, dim=0, weights=w)
    le = sym.sym_expm((w[:, None, None] * sym.sym_logm(x)).sum(0))
    # ten spectral functions on the path (logm, expm, the last step's five logmaps and expmap), each within
    # C n eps cond ||A|| of its own result; cond <= 8 and ||A|| <= 4 here
    tol = 10 * P.C * n * eps * 8.0 * 4.0
    assert got.shape == le.shape
    assert (_err(dn, n, num(got), num(le)) <= tol).all()
    assert (_err(dn, n, num(sym.sym_karcher_mean(x.transpose(0, 1), dim=1, weights=w)), num(got)) <= tol).all()
    # two matrices: the geometric mean
    ca, cb, cells = P.batch(dn, n, 'sqrt')
    sl = cells['normal']
    pair = torch.stack([T(dev, ca[sl]), T(dev, cb[sl])])
    gm = sym.sym_geomean(pair[0], pair[1])
    m = P.model(dn, 'sqrt', ca[sl], cb[sl])
    # (the iteration converges linearly from the log-Euclidean start: 32 steps reach the float64 rounding level)
    km = sym.sym_karcher_mean(pair, max_iter=32)
    assert (_err(dn, n, num(km), num(gm)) <= 10 * P.C * P.fun_bound(dn, 'sqrt', m)).all()
    # a well-conditioned set of 5 x 256: the gradient of the Karcher functional vanishes after max_iter steps.
    # The step-one iteration contracts by a factor that grows with the squared geodesic diameter of the set; the
    # members are within 0.25 of a common centre (A_i = S exp(E_i) S, ||E_i||_F <= 0.25), a neighbourhood of a
    # tensor field, for which the default 8 steps reach the rounding level in both dtypes
    centre = R.family('normal', dn, rng, 256, n)
    root = P._sqrt_spd(centre)
    members = []
    for _ in range(5):
        e = P._sym(rng.standard_normal((256, n, n)))
        e *= (0.25 * rng.uniform(0.2, 1.0, (256, 1, 1))) / np.sqrt((e * e).sum((1, 2), keepdims=True))
        lam, v = np.linalg.eigh(e)
        members.append(P._sym(root @ np.einsum('bik,bk,bjk->bij', v, np.exp(lam), v) @ root))
    y = T(dev, R.pack(np.stack(members)).astype(R.NP[dn]))
    mean = sym.sym_karcher_mean(y, weights=w)
    resid = (w[:, None, None] * sym.sym_logmap(mean.unsqueeze(0).expand(y.shape), y)).sum(0)
    norm = R._fro(R.unpack(num(resid).astype(np.float64), n))
    print(f'{dn}: Karcher residual {norm.max() / (n * eps):.1f} n eps (of {P.C} x cond, cond <= 10)')
    assert (norm <= P.C * n * eps * 10.0).all()
