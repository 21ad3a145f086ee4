"""The Frechet kernels of `lie.expm` (`ExpmFrechetOp<T, D, DEPTH>`: two dtypes, orders 1..4, L and L2) on the MI355X:
accuracy per record on every input class, closed forms, batch sizes and layouts bit for bit, the facade with a
per-record basis, the backward, truncated series, non-finite and extreme input.

Truths, the reference, the model, the unit D eps (1 + ||X||_1) and the constant C = max(4, 2 C_ref) are those of
tests/_lie_ref.py (its bounds are shown attainable on the CPU by test_lie_host.py).  Every record gets its own
verdict; a failure names the class, the record and error / unit."""
import pytest
import torch
import _lie_ref as R

pytestmark = pytest.mark.gpu

DNS = ('f32', 'f64')
N_ACC = 2000
C_BACKWARD = 4          # test_gpu_lie.C_DERIV, on the unit D eps (1 + ||X||_1)^2


@pytest.fixture(scope='module')
def lie():
    from nitorch_fastmath_amd import lie
    return lie


def fr(lie, X, A, B=None, max_order=10000, tol=1e-32):
    return lie._frechet(X, A, B, max_order, tol)


def frechet_tile(dn, D, depth):
    """ExpmFrechetOp::TILE = pick_tile((DEPTH + 1) D^2 sizeof(T) + 16), pick_tile(b) = 256 if 256 b <= 36 KiB,
    128 if 128 b <= 36 KiB, else 64 (nfm_common.hpp): 256 lanes up to 144 bytes, 128 up to 288.
    float32: 256 everywhere except L2 at D = 4 (208 bytes: 128).  float64: 256 at D = 1, 2; 128 at D = 3 (160 and
    232 bytes) and for L at D = 4 (272); 64 for L2 at D = 4 (400 bytes)."""
    b = (depth + 1) * D * D * (4 if dn == 'f32' else 8) + 16
    return 256 if b * 256 <= 36 * 1024 else (128 if b * 128 <= 36 * 1024 else 64)


# ------------------------------------------------------------------------------------------ a. accuracy per record
@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_accuracy_float32(lie, D, depth):
    """2000 records of every class against the float64 truth, the bar set by the float32 reference"""
    x, a, b, where = R.all_inputs(N_ACC, D, 'f32')
    b = b if depth == 2 else None
    k = fr(lie, x.cuda(), a.cuda(), None if b is None else b.cuda()).cpu()
    R.class_verdicts(k, R.frechet_truth64(x, a, b), R.frechet_ref(x, a, b, torch.float32), x, torch.float32, where,
                     f'float32 D={D} L{depth}', show=True)


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('D', [2, 3, 4])
def test_accuracy_float64_fixture(lie, D, depth):
    """the 96 records of the 40-digit fixture (one and a half wavefronts), the bar set by the float64 reference"""
    x, a, b, L, L2 = R.fixture_records(D)
    bb = b if depth == 2 else None
    k = fr(lie, x.cuda(), a.cuda(), None if bb is None else bb.cuda()).cpu()
    R.class_verdicts(k, L2 if depth == 2 else L, R.frechet_truth64(x, a, bb), x, torch.float64, R.fixture_classes(),
                     f'float64 fixture D={D} L{depth}', show=True)


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_accuracy_float64(lie, D, depth):
    """2000 records of every class against the float64 block identities, whose own error is of the same order:
    twice the constant (as test_gpu_lie.test_scale), the constant being that of the fixture's class at this order"""
    x, a, b, where = R.all_inputs(N_ACC, D, 'f64')
    b = b if depth == 2 else None
    k = fr(lie, x.cuda(), a.cuda(), None if b is None else b.cuda()).cpu()
    ck = R.c_of(k, R.frechet_truth64(x, a, b), x, torch.float64)
    msgs = []
    for cls, sl in where:
        cmax = 2 * R.c_bound(R.fixture_c_ref(D, depth)[cls] if D > 1 else 0.0, D)
        print(f'float64 D={D} L{depth} {R.cname(cls)}: kernel {float(ck[sl].max()):.2f} bound {cmax:.2f} units')
        msgs.append(R.verdict(ck[sl], cmax, f'float64 D={D} L{depth} {R.cname(cls)}'))
    assert not any(msgs), '\n'.join(m for m in msgs if m)


# ------------------------------------------------------------------------------------------ b. closed forms
N_CF = 300
CF_CLASS = ('gen', 2.0)           # the class whose constant the closed forms without a class of their own are held to


def class_constant(cls, D, dn, depth, n=N_CF):
    """max(4, 2 C_ref) of a class on n of its records (float64: the fixture's constant, twice)"""
    if dn == 'f64':
        return 2 * R.c_bound(R.fixture_c_ref(D, depth)[cls] if D > 1 else 0.0, D)
    x, a, b = R.inputs(cls, n, D, dn)
    b = b if depth == 2 else None
    return R.c_bound(R.c_of(R.frechet_ref(x, a, b, R.DT[dn]), R.frechet_truth64(x, a, b), x, R.DT[dn]).max(), D)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_closed_forms(lie, dn, D):
    dtype = R.DT[dn]
    x, a, b = (t.cuda() for t in R.inputs(CF_CLASS, N_CF, D, dn))
    ad, bd = a.double().cpu(), b.double().cpu()
    sym = (ad @ bd + bd @ ad) / 2
    c1, c2 = (class_constant(CF_CLASS, D, dn, depth) for depth in (1, 2))
    # X = 0: L = A bit for bit, L2 = (AB + BA) / 2
    z = torch.zeros_like(x)
    assert torch.equal(fr(lie, z, a), a)
    R.held(fr(lie, z, a, b), sym, z, dtype, c2, f'{dn} D={D} L2 at X = 0')
    # X = c I: L = e^c A, L2 = e^c (AB + BA) / 2
    for c in (-3.0, 0.5, 6.0):
        xi = (c * torch.eye(D, dtype=dtype)).expand(N_CF, D, D).contiguous().cuda()
        ec = torch.exp(torch.tensor(c, dtype=dtype).double())
        R.held(fr(lie, xi, a), ec * ad, xi, dtype, c1, f'{dn} D={D} L at X = {c} I')
        R.held(fr(lie, xi, a, b), ec * sym, xi, dtype, c2, f'{dn} D={D} L2 at X = {c} I')
    # A = X: L = X expm(X) = expm(X) X
    ex = torch.linalg.matrix_exp(x.double().cpu())
    k = fr(lie, x, x)
    R.held(k, x.double().cpu() @ ex, x, dtype, c1, f'{dn} D={D} L(X, X) = X expm(X)')
    R.held(k, ex @ x.double().cpu(), x, dtype, c1, f'{dn} D={D} L(X, X) = expm(X) X')
    # L2 symmetric in its directions: to the bound (the two orders round differently), each against the truth too
    t2 = R.frechet_truth64(x, a, b)
    kab, kba = fr(lie, x, a, b), fr(lie, x, b, a)
    R.held(kab, t2, x, dtype, c2, f'{dn} D={D} L2(X, A, B)')
    R.held(kba, t2, x, dtype, c2, f'{dn} D={D} L2(X, B, A)')
    R.held(kab, kba.double(), x, dtype, 2 * c2, f'{dn} D={D} L2(X, A, B) against L2(X, B, A)')
    # linearity in A: a power of two commutes with every step, bit for bit
    for e in (-20, 7):
        assert torch.equal(fr(lie, x, a * 2.0 ** e), fr(lie, x, a) * 2.0 ** e), (dn, D, e)
        assert torch.equal(fr(lie, x, a * 2.0 ** e, b), kab * 2.0 ** e), (dn, D, e)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('D', [2, 3, 4])
def test_nilpotent_finite_sum(lie, dn, D):
    """strictly upper triangular X: the series ends at X^(D-1), the double (triple) sum is exact"""
    dtype = R.DT[dn]
    for cls in (('nilp', 1.0), ('nilp', 5.0)):
        x, a, b = R.inputs(cls, N_CF, D, dn)
        for depth in (1, 2):
            bb = b if depth == 2 else None
            k = fr(lie, x.cuda(), a.cuda(), None if bb is None else bb.cuda())
            R.held(k, R.series_frechet(x, a, bb), x, dtype, class_constant(cls, D, dn, depth),
                   f'{dn} D={D} L{depth} {R.cname(cls)} finite sum')


@pytest.mark.parametrize('dn', DNS)
def test_scalars(lie, dn):
    """D = 1: exp(x) a and exp(x) a b"""
    dtype = R.DT[dn]
    for cls in (('gen', 1e-3), ('gen', 2.0), ('gen', 30.0)):
        x, a, b = R.inputs(cls, N_CF, 1, dn)
        ex = torch.exp(x.double())
        R.held(fr(lie, x.cuda(), a.cuda()), ex * a.double(), x, dtype, R.C_FLOOR, f'{dn} scalar L {R.cname(cls)}')
        R.held(fr(lie, x.cuda(), a.cuda(), b.cuda()), ex * a.double() * b.double(), x, dtype, R.C_FLOOR,
               f'{dn} scalar L2 {R.cname(cls)}')


# ------------------------------------------------------------------------------------------ c. sizes and layouts
@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('D', [1, 3, 4])
def test_batch_sizes_bit_for_bit(lie, dn, D, depth):
    """a record's result does not depend on the launch it is in: every size against the first records of one large
    launch, and the middle record against a launch of its own.  Sizes: 1, around a wavefront, several workgroups,
    and one under, at and one over every record tile the op can have (64, 128, 256: `frechet_tile`)"""
    tile = frechet_tile(dn, D, depth)
    sizes = sorted({1, 63, 64, 65, 257, 1001, 127, 128, 129, 255, 256, tile - 1, tile, tile + 1})
    x, a, b = (t[:1001].cuda() for t in R.inputs(('gen', 8.0), N_ACC, D, dn))
    b = b if depth == 2 else None
    big = fr(lie, x, a, b)
    R.held(big, R.frechet_truth64(x, a, b), x, R.DT[dn], class_constant(('gen', 8.0), D, dn, depth),
           f'{dn} D={D} L{depth} 1001 records')
    for n in sizes:
        out = fr(lie, x[:n], a[:n], None if b is None else b[:n])
        assert torch.equal(out, big[:n]), (n, int((out != big[:n]).any(-1).any(-1).nonzero()[0]))
        h = n // 2
        one = fr(lie, x[h:h + 1], a[h:h + 1], None if b is None else b[h:h + 1])
        assert torch.equal(one[0], big[h]), (n, h)


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('D', [1, 3, 4])
def test_layouts_bit_for_bit(lie, dn, D, depth):
    """every layout of X and of the directions against the contiguous call on the same values"""
    dtype = R.DT[dn]
    n = 301
    gen = torch.Generator().manual_seed(11 * D + depth)
    xp, ap, bp = (torch.randn(n, D, D + 1, dtype=dtype, generator=gen).cuda() for _ in range(3))
    xp = xp * 0.9                                             # ||X||_1 around 2 to 4: a few squarings
    X, A, B = xp[..., :D], ap[..., :D], bp[..., :D]           # records padded to D x (D + 1)
    two = depth == 2

    def f(x, a, b):
        return fr(lie, x, a, b if two else None)

    def c(t, shape=None):
        return (t if shape is None else t.expand(shape)).contiguous()

    ref = f(c(X), c(A), c(B))
    full = (n, D, D)
    cases = {
        'padded records': (X, A, B),
        'X transposed by strides': (c(X.mT).mT, c(A), c(B)),
        'directions transposed by strides': (c(X), c(A.mT).mT, c(B.mT).mT),
        'every other record': (X[::2], A[::2], B[::2]),
        'two batch levels': (X.reshape(7, 43, D, D), A.reshape(7, 43, D, D), B.reshape(7, 43, D, D)),
        'X with stride 0': (X[:1].expand(full), c(A), c(B)),
        'X unbatched': (c(X[0]), c(A), c(B)),
        'A broadcast': (c(X), A[:1], c(B)),
        'B broadcast': (c(X), c(A), B[:1].expand(full)),
        'packed X, padded directions': (c(X), A, B),
    }
    want = {
        'every other record': ref[::2],
        'two batch levels': ref.reshape(7, 43, D, D),
        'X with stride 0': f(c(X[:1], full), c(A), c(B)),
        'X unbatched': f(c(X[:1], full), c(A), c(B)),
        'A broadcast': f(c(X), c(A[:1], full), c(B)),
        'B broadcast': f(c(X), c(A), c(B[:1], full)),
    }
    for name, (x, a, b) in cases.items():
        out = f(x, a, b)
        assert out.is_contiguous(), name
        assert torch.equal(out, want.get(name, ref)), (name, dn, D, depth)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = f(c(X), c(A), c(B))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(side, ref)


# ------------------------------------------------------------------------------------------ d. the facade
@pytest.mark.parametrize('D', [2, 4])
def test_facade_per_record_basis(lie, D):
    """`expm_derivatives` with a basis per record (n, F, D, D): dX, dB and every entry of hX -- the lower half, which
    the facade fills by copying, against an independent L2(M, B_g, B_f)"""
    n, F = 70, 5
    gen = torch.Generator().manual_seed(D)
    basis = torch.randn(n, F, D, D, dtype=torch.float64, generator=gen) * 0.5
    p = torch.randn(n, F, dtype=torch.float64, generator=gen)
    e, dX, dB, hX = lie.expm_derivatives(p.cuda(), basis.cuda(), grad_X=True, grad_basis=True, hess_X=True)
    assert dX.shape == (n, F, D, D) and dB.shape == (n, F, D, D, D, D) and hX.shape == (n, F, F, D, D)
    M = torch.einsum('nf,nfij->nij', p, basis)
    Mx = M[:, None]
    c1, c2 = (2 * R.c_bound(max(R.fixture_c_ref(D, depth).values()), D) for depth in (1, 2))
    R.held(e, torch.linalg.matrix_exp(M), M, torch.float64, c1, f'D={D} E')
    R.held(dX, R.frechet_truth64(Mx, basis), Mx.expand(n, F, D, D), torch.float64, c1, f'D={D} dX')
    for f in range(F):
        for g in range(F):
            R.held(hX[:, f, g], R.frechet_truth64(M, basis[:, g], basis[:, f]), M, torch.float64, c2,
                   f'D={D} hX[:, {f}, {g}]')
    one = torch.eye(D * D, dtype=torch.float64).reshape(D * D, D, D)
    Lij = R.frechet_truth64(Mx, one).reshape(n, 1, D, D, D, D)
    t = p.reshape(n, F, 1, 1, 1, 1) * Lij
    k = dB.cpu()
    # per record and parameter: x_f L(M, e_ij) over all (i, j), on the scale of its largest entry
    d = (k - t).abs().amax((-4, -3, -2, -1)) / t.abs().amax((-4, -3, -2, -1))
    c = d / R.unit(M, torch.float64)[:, None]
    msg = R.verdict(c, c1, f'D={D} dB')
    assert msg is None, msg


@pytest.mark.parametrize('D', [2, 3, 4, 5])
def test_facade_float32(lie, D):
    """float32 through the facade: the kernels at D = 2, 3, 4, the torch route at D = 5, one bar"""
    n = 70
    x = R.inputs(('gen', 2.0), n, D, 'f32')[0]
    e, dX, hX = lie.expm_derivatives(x.cuda(), grad_X=True, hess_X=True)
    F = D * D
    one = torch.eye(F, dtype=torch.float32).reshape(F, D, D)
    Mx = x[:, None]
    Mf = Mx.expand(n, F, D, D)
    t1 = R.frechet_truth64(Mx, one)
    c1 = R.c_bound(R.c_of(R.frechet_ref(Mx, one, None, torch.float32), t1, Mf, torch.float32).max(), D)
    R.held(dX, t1, Mf, torch.float32, c1, f'float32 D={D} dX')
    for f in range(0, F, 3):
        t2 = R.frechet_truth64(Mx, one[f], one)
        c2 = R.c_bound(R.c_of(R.frechet_ref(Mx, one[f], one, torch.float32), t2, Mf, torch.float32).max(), D)
        R.held(hX[:, f], t2, Mf, torch.float32, c2, f'float32 D={D} hX[:, {f}]')


# ------------------------------------------------------------------------------------------ e. the backward
@pytest.mark.parametrize('nrm', [0.5, 8.0])
@pytest.mark.parametrize('dn,D', [('f32', D) for D in (1, 2, 4, 5, 8)] + [('f64', D) for D in (2, 4, 7)])
def test_backward(lie, dn, D, nrm):
    """autograd through `lie.expm` (the kernel at D <= 4, the torch route above) against the float64 autograd of
    matrix_exp, per record, on the unit D eps (1 + ||X||_1)^2 of test_grad_matches_matrix_exp_float32; float64 is
    compared with an algorithm of its own precision: twice the constant"""
    dtype = R.DT[dn]
    n = 1000
    gen = torch.Generator().manual_seed(D)
    x = R.build_x(('gen', nrm), n, D, gen).to(dtype).cuda().requires_grad_()
    g = torch.randn(n, D, D + 1, dtype=dtype, generator=gen).cuda()[..., :D].mT       # non-contiguous
    assert not g.is_contiguous() or D == 1
    (gk,) = torch.autograd.grad(lie.expm(x), x, g)
    x64 = x.detach().double().requires_grad_()
    (gt,) = torch.autograd.grad(torch.linalg.matrix_exp(x64), x64, g.double())
    n1 = R.norm1(x.detach().cpu())
    c = R.err(gk, gt) / (D * torch.finfo(dtype).eps * (1 + n1) ** 2)
    cmax = C_BACKWARD if dn == 'f32' else 2 * C_BACKWARD
    print(f'backward {dn} D={D} norm {nrm}: worst {float(c.max()):.2f} of {cmax} units')
    msg = R.verdict(c, cmax, f'backward {dn} D={D} gen-{nrm:g}')
    assert msg is None, msg


# ------------------------------------------------------------------------------------------ f. max_order and tol
@pytest.mark.parametrize('limits', [(1, 1e-32), (2, 1e-32), (5, 1e-32), (10000, 1e-4), (10000, 1e-12)])
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('D', [2, 3, 4])
def test_truncated_series(lie, dn, D, limits):
    """`max_order` and `tol` reach the derivative kernels: the value of the truncated series, from the model in
    float64 with the squarings and the degree pinned to those of the dtype under test.  A record whose term bound is
    within 1e-3 of the limit (the kernel's ||Y||_F is rounded differently: at most D^2 eps on a 20th power) may
    take the neighbouring degree: it is held to the nearer of the two values."""
    max_order, tol = limits
    dtype = R.DT[dn]
    for cls in (('gen', 0.5), ('gen', 8.0)):
        x, a, b = R.inputs(cls, N_CF, D, dn)
        for depth in (1, 2):
            bb = b if depth == 2 else None
            k = fr(lie, x.cuda(), a.cuda(), None if bb is None else bb.cuda(), max_order, tol)
            c = R.truncated_verdict(k, x, a, bb, dtype, max_order, tol)
            msg = R.verdict(c, class_constant(cls, D, dn, depth), f'{dn} D={D} L{depth} {R.cname(cls)} '
                            f'max_order={max_order} tol={tol:g}')
            assert msg is None, msg


# ------------------------------------------------------------------------------------------ g. non-finite, extreme
def same(x, y):
    return bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('D', [1, 2, 4])
def test_non_finite_and_extreme(lie, dn, D, depth):
    dtype = R.DT[dn]
    n = 131
    x, a, b = (t[:n].clone() for t in R.inputs(('gen', 2.0), N_CF, D, dn))
    ops = [x, a] + ([b] if depth == 2 else [])

    def run(ts):
        return fr(lie, *[t.cuda() for t in ts]).cpu()

    clean = run(ops)
    assert torch.isfinite(clean).all()
    spots = (0, 63, 64, 130)                         # first lane, both sides of a wavefront, the last record
    for which in range(len(ops)):
        for bad in (float('nan'), float('inf'), -float('inf')):
            ts = [t.clone() for t in ops]
            for r in spots:
                ts[which][r, D - 1, 0] = bad
            out = run(ts)
            rest = torch.ones(n, dtype=torch.bool)
            rest[list(spots)] = False
            assert torch.isnan(out[list(spots)]).all(), (which, bad)
            assert torch.equal(out[rest], clean[rest]), (which, bad)
    # huge and finite: the call returns (overflow allowed), the neighbours do not notice
    for which in range(len(ops)):
        ts = [t.clone() for t in ops]
        ts[which][64] = torch.finfo(dtype).max / 8
        out = run(ts)
        rest = torch.arange(n) != 64
        assert torch.equal(out[rest], clean[rest]), which
    # denormal X: L = A, L2 = (AB + BA) / 2 to the bound
    xd = torch.full_like(x, torch.finfo(dtype).tiny / 64)
    want = a.double() if depth == 1 else (a.double() @ b.double() + b.double() @ a.double()) / 2
    R.held(run([xd] + ops[1:]), want, xd, dtype, R.C_FLOOR, f'{dn} D={D} L{depth} denormal X')
