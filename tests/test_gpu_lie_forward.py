"""The forward kernels of `lie.expm` (`ExpmOp<T, D>`: float32 orders 1..8, float64 orders 1..7) on the MI355X: a
conditioning bound per record on every input class, lanes of a wavefront with different trip counts, `max_order` and
`tol` through `nfm_lie_expm`, and the overflow edge.

Classes, truths, the model and the unit D eps max(1, cond_exp(X)) on the Frobenius error are those of
tests/_lie_ref.py (shown attainable at C_EXPM / 2 on the CPU by test_lie_host.py); the constant is test_gpu_lie.py's
C_EXPM.  Every record gets its own verdict; a failure names the class, the record and error / unit."""
import pytest
import torch
import _lie_ref as R
from test_gpu_lie import C_EXPM
from nitorch_fastmath_amd.lie import FORWARD_MAX

pytestmark = pytest.mark.gpu

CASES = [(dn, D) for dn in ('f32', 'f64') for D in range(1, FORWARD_MAX[R.DT[dn]] + 1)]


@pytest.fixture(scope='module')
def lie():
    from nitorch_fastmath_amd import lie
    return lie


def same_bits(a, b):
    return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                       b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


# ------------------------------------------------------------------------------------------ a. bounds per record
@pytest.mark.parametrize('dn,D', CASES)
def test_per_record_bounds(lie, dn, D):
    """one batch per (dtype, order), record i of class i mod C: every wavefront holds every (s, m), from (0, 5) to
    (10, 22).  float32: 768 records against matrix_exp in float64; float64: the 120 records of
    the 40-digit fixture, at order 1 exp in float64.  Every record finite and within C_EXPM units.  Printed beside
    it, setting no bar: torch.linalg.matrix_exp in the same dtype on the CPU."""
    dtype = R.DT[dn]
    x, idx, t, cond = R.fwd_case(D, dn)
    classes = R.fwd_classes(dn, D)
    k = lie.expm(x.cuda()).cpu()
    ck = R.fwd_c(k, t, x, dtype, cond)
    cr = R.fwd_c(torch.linalg.matrix_exp(x) if D > 1 else torch.exp(x), t, x, dtype, cond)
    wk, wr = R.fwd_worst(ck, idx, classes), R.fwd_worst(cr, idx, classes)
    for name in wk:
        print(f'forward {dn} D={D} {name}: kernel {wk[name]:.2f} matrix_exp {wr[name]:.2f} units')
    bad = torch.nonzero(~torch.isfinite(k).all(-1).all(-1)).reshape(-1)
    assert bad.numel() == 0, f'{dn} D={D}: records {bad[:8].tolist()} are not finite'
    R.fwd_verdicts(ck, idx, classes, C_EXPM, f'forward {dn} D={D}')


# ------------------------------------------------------------------------------------------ b. lanes
@pytest.mark.parametrize('dn,D', CASES)
def test_lanes_are_independent(lie, dn, D):
    """both loops of ExpmOp are per lane: a record among neighbours of every other (s, m) has the bits it has in a
    batch of its own class, where every lane runs nearly the same trip counts -- at every cut of the batch"""
    x, idx = R.fwd_batch(R.FWD_N, D, dn)
    xg = x.cuda()
    own = torch.empty_like(xg)
    for q in range(len(R.fwd_classes(dn, D))):
        rec = torch.nonzero(idx == q).reshape(-1).cuda()
        own[rec] = lie.expm(xg[rec].contiguous())
    assert torch.isfinite(own).all()
    for n in (1, 63, 64, 65, 257, R.FWD_N):
        out = lie.expm(xg[:n])
        diff = torch.nonzero((out != own[:n]).any(-1).any(-1)).reshape(-1)
        assert diff.numel() == 0, (dn, D, n, diff[:8].tolist())
        assert same_bits(out, own[:n])


# ------------------------------------------------------------------------------------------ c. max_order and tol
TRUNC_CASES = [('f32', D) for D in (2, 4, 5, 8)] + [('f64', D) for D in (2, 4, 7)]
TRUNC_CLASSES = (('gen', 0.5), ('gen', 8.0), ('gen', 30.0), ('nilp', 5.0))
N_TRUNC = 64


@pytest.mark.parametrize('limits', [(1, 1e-32), (2, 1e-32), (5, 1e-32), (10000, 1e-4), (10000, 1e-12), (10000, 0.0)])
@pytest.mark.parametrize('dn,D', TRUNC_CASES)
def test_truncated_series(lie, dn, D, limits):
    """`max_order` and `tol` reach `nfm_lie_expm`: the value of the truncated series, from `expm_model` in float64
    with the squarings and the degree pinned to those of the dtype under test, in C_EXPM units of D eps (1 + ||X||_1)
    (the model is the truth here, so conditioning does not enter).  A record whose term bound is within 1e-3 of the
    limit may take the neighbouring degree: it is held to the nearer of the two values."""
    max_order, tol = limits
    dtype = R.DT[dn]
    for cls in TRUNC_CLASSES:
        x = R.fwd_inputs(cls, N_TRUNC, D, dn)
        k = lie.expm(x.cuda(), max_order=max_order, tol=tol).cpu()
        c = R.truncated_verdict(k, x, None, None, dtype, max_order, tol)
        print(f'truncated {dn} D={D} {R.cname(cls)} max_order={max_order} tol={tol:g}: worst {float(c.max()):.2f} units')
        msg = R.verdict(c, C_EXPM, f'{dn} D={D} {R.cname(cls)} max_order={max_order} tol={tol:g}')
        assert msg is None, msg


@pytest.mark.parametrize('dn,D', TRUNC_CASES)
def test_truncation_shows(lie, dn, D):
    """the test above can tell whether the arguments arrived: on the gen-30 records the series cut at degree 5 is
    not the default result.  The cut moves a record by ||Y^6|| / 6! 2^s, which depends on its spectrum, not on its
    norm: in float64 every record moves by thousands of units, in float32 (`expm_model` in float64, 64 records) the
    median record moves by 23 units at order 2, 7 at order 4, 1.7 at order 5 and 0.4 at order 8, the worst by 1700,
    270, 51 and 7.3.  So: the worst record differs by more than C_EXPM units, and so does every record that the
    model moves by more than 3 C_EXPM (each of the two results may be C_EXPM off its own value).  `expm_derivatives`
    hands the same limits to the same kernel: bit for bit."""
    dtype = R.DT[dn]
    x = R.fwd_inputs(('gen', 30.0), N_TRUNC, D, dn)
    xg = x.cuda()
    full, cut = lie.expm(xg), lie.expm(xg, max_order=5, tol=1e-32)
    c = R.c_of(cut, full.double().cpu(), x, dtype)
    full64 = R.expm_model(x, torch.float64, plan=R.lie_plan(x)[:2])[0]
    cut64 = R.expm_model(x, torch.float64, plan=R.lie_plan(x, 5, 1e-32)[:2])[0]
    moved = R.c_of(cut64, full64, x, dtype) > 3 * C_EXPM
    print(f'truncation {dn} D={D}: worst {float(c.max()):.3g} units, {int(moved.sum())} of {N_TRUNC} records past '
          f'3 C_EXPM in the model, the least of them at {float(c[moved].min()) if bool(moved.any()) else 0:.3g}')
    assert float(c.max()) > C_EXPM
    assert bool((c[moved] > C_EXPM).all())
    if dn == 'f64':
        assert bool(moved.all())
    two = lie.expm(xg, max_order=2)
    assert not torch.equal(two, full)
    if D <= lie.FRECHET_MAX:
        assert same_bits(lie.expm_derivatives(xg, grad_X=True, max_order=2)[0], two)
    assert same_bits(lie.expm_derivatives(xg, max_order=2), two)
    assert same_bits(lie.expm_derivatives(xg, max_order=10000, tol=1e-4), lie.expm(xg, tol=1e-4))


# ------------------------------------------------------------------------------------------ d. the overflow edge
SPOTS = (3, 31, 63, 64, 90, 127)             # over two wavefronts: first and last lanes, and some in between


def overflowing(D, dn, nrm):
    """six general records of ||X||_1 = nrm, rounded to the dtype, whose exponential (float64 on the host) overflows
    the dtype, and no entry of it within a factor 4 of the dtype's maximum: which entries overflow is beyond doubt"""
    dtype = R.DT[dn]
    big = torch.finfo(dtype).max
    x = R.fwd_inputs(('gen', nrm), 64, D, dn, salt=7)
    t = R.fwd_truth64(x).abs()
    assert torch.isfinite(t).all()
    pick = (t.amax((-2, -1)) > 4 * big) & ~((t > big / 4) & (t < 4 * big)).any(-1).any(-1)
    rec = torch.nonzero(pick).reshape(-1)[:len(SPOTS)]
    assert rec.numel() == len(SPOTS)
    return x[rec], t[rec] > big


def check_overflow(lie, dn, D, xo, over):
    x = R.fwd_batch(R.FWD_N, D, dn)[0]
    clean = lie.expm(x.cuda()).cpu()
    assert torch.isfinite(clean).all()
    x = x.clone()
    x[list(SPOTS)] = xo
    out = lie.expm(x.cuda()).cpu()
    torch.cuda.synchronize()
    assert bool(over.any(-1).any(-1).all())
    assert not bool(torch.isfinite(out[list(SPOTS)])[over].any()), (dn, D)
    rest = torch.ones(R.FWD_N, dtype=torch.bool)
    rest[list(SPOTS)] = False
    assert same_bits(out[rest], clean[rest]), (dn, D)


@pytest.mark.parametrize('D', [4, 8])
def test_overflow_edge_float32(lie, D):
    """records whose exponential leaves float32 (||X||_1 = 400: s = 9) among the interleaved batch: not finite
    wherever the truth is past the maximum, and no other record notices"""
    xo, over = overflowing(D, 'f32', 400.0)
    check_overflow(lie, 'f32', D, xo, over)


def test_overflow_edge_float64(lie):
    """the same in float64 at ||X||_1 = 3000 (s = 12), the records and log2 |e^X| from the 40-digit fixture"""
    g = R.fwd_fixture()
    xo, over = torch.from_numpy(g['over_x_4']), torch.from_numpy(g['over_log2_4']) > 1024
    check_overflow(lie, 'f64', 4, xo, over)
