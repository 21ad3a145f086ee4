"""Truths, a model and per-record verdicts for the Frechet derivatives of `lie.expm` (shared by test_lie_host.py and
test_gpu_lie_derivatives.py).  Plain torch on the CPU; nothing here touches the kernels.

    frechet_truth64   the block identities of lie.py's docstring through `torch.linalg.matrix_exp` in float64, on the
                      dtype-rounded inputs: the truth for float32 results (its own error, 1e-15 (1 + ||X||_1), is
                      checked against a 40-digit fixture by test_lie_host.py)
    frechet_ref       the same identities evaluated in the dtype under test: an independent algorithm (Pade) of the
                      same precision, whose error sets the bar
    frechet_model     a transcription of the algorithm in the header of nfm_lie_ops.hpp (scaling, degree, three
                      coupled Horner recurrences, squarings): shows that the bars are attainable and gives the value
                      of a truncated series.  A model of the formulas, not of the fma order: nothing is held to its bits.
    expm_model        the forward part of that transcription, E alone: the same for `ExpmOp`

The forward kernels have classes, a conditioning unit (`cond_exp`, `fwd_unit`, `fwd_c`) and a 40-digit fixture of
their own in the last section (test_gpu_lie_forward.py).

Every measure is ONE NUMBER PER RECORD.  Error of a result K against a truth T: max|K - T| / max|T|; the unit is
D eps (1 + ||X||_1), the project's own (profiles/expm_accuracy.md).  A kernel is held to C units with
C = max(4, 2 C_ref), C_ref the worst error / unit of `frechet_ref` on the same inputs against the same truth: 4 is
the constant of test_gpu_lie.py, and a Taylor-Horner scheme may be the worse of two algorithms of the same order by
a small factor, not by an order.  A class whose C_ref exceeds C_REF_CAP is not a usable class.
"""
import functools
import os
import numpy as np
import torch
from conftest import GOLDEN

DT = {'f32': torch.float32, 'f64': torch.float64}
NORMS = (1e-3, 0.5, 2.0, 8.0, 30.0)          # ||X||_1 of the general classes (as tests/golden/make_golden_lie.py)
SKEW_NORMS = (4.0, 20.0, 200.0)              # the exponential stays bounded: s reaches 8 without overflow in float32
NILP_NORMS = (1.0, 5.0)
CLASSES = tuple(('gen', v) for v in NORMS) + tuple(('skew', v) for v in SKEW_NORMS) + \
    tuple(('nilp', v) for v in NILP_NORMS)
FIXTURE_COUNT = {'gen': 12, 'skew': 6, 'nilp': 9}        # records per class and order in golden/lie_frechet.npz
FIXTURE_ORDERS = (2, 3, 4)
C_FLOOR = 4.0
C_REF_CAP = 8.0
MAX_SQUARINGS = 64                           # kLieMaxSquarings


def cname(cls):
    return f'{cls[0]}-{cls[1]:g}'


# ------------------------------------------------------------------------------------------ inputs
def _seed(cls, D, salt):
    kinds = {'gen': 1, 'skew': 2, 'nilp': 3, 'shift': 4, 'tri': 5, 'edge': 6}
    return torch.Generator().manual_seed(int(kinds[cls[0]] * 1000003 + round(cls[1] * 1000) * 101 + D * 7 + salt * 13))


def build_x(cls, n, D, gen):
    """n float64 matrices of a class, ||X||_1 = the class norm (order 1: a skew-symmetric or strictly upper
    triangular matrix is zero)"""
    kind, nrm = cls
    g = torch.randn(n, D, D, dtype=torch.float64, generator=gen)
    if kind == 'skew':
        g = g - g.mT
    elif kind == 'nilp':
        g = torch.triu(g, 1)
    n1 = g.abs().sum(-2).amax(-1)
    return g * (nrm / torch.where(n1 > 0, n1, torch.ones_like(n1)))[:, None, None]


@functools.lru_cache(maxsize=None)
def inputs(cls, n, D, dn, salt=0):
    """(X, A, B) of a class, rounded to the dtype `dn` ('f32' / 'f64'); shared, not to be written to"""
    gen = _seed(cls, D, salt)
    x = build_x(cls, n, D, gen)
    a = torch.randn(n, D, D, dtype=torch.float64, generator=gen)
    b = torch.randn(n, D, D, dtype=torch.float64, generator=gen)
    return tuple(t.to(DT[dn]) for t in (x, a, b))


@functools.lru_cache(maxsize=None)
def all_inputs(n, D, dn, salt=0, first=None):
    """every class, n records each, in one batch: (X, A, B, [(class, slice), ...]); `first` keeps the first records
    of each class only (the same records, not a smaller draw)"""
    k = n if first is None else first
    parts = [tuple(t[:k] for t in inputs(cls, n, D, dn, salt)) for cls in CLASSES]
    where = [(cls, slice(i * k, (i + 1) * k)) for i, cls in enumerate(CLASSES)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3)) + (where,)


# ------------------------------------------------------------------------------------------ truths
def _blocks(X, A, B, dtype):
    X, A = X.to(dtype), A.to(dtype)
    D = X.shape[-1]
    shapes = [X.shape[:-2], A.shape[:-2]] + ([] if B is None else [B.shape[:-2]])
    batch = torch.broadcast_shapes(*shapes)
    k = 2 if B is None else 4
    Z = torch.zeros(tuple(batch) + (k * D, k * D), dtype=dtype)
    for q in range(k):
        Z[..., q * D:(q + 1) * D, q * D:(q + 1) * D] = X
    if B is None:
        Z[..., :D, D:] = A
        return Z, (slice(0, D), slice(D, 2 * D))
    B = B.to(dtype)
    Z[..., :D, D:2 * D] = A
    Z[..., :D, 2 * D:3 * D] = B
    Z[..., D:2 * D, 3 * D:] = B
    Z[..., 2 * D:3 * D, 3 * D:] = A
    return Z, (slice(0, D), slice(3 * D, 4 * D))


def frechet_ref(X, A, B, dtype):
    """L(X, A) (B None) or L2(X, A, B) by the block identities, evaluated in `dtype` on the CPU"""
    Z, (r, c) = _blocks(X.cpu(), A.cpu(), None if B is None else B.cpu(), dtype)
    return torch.linalg.matrix_exp(Z)[..., r, c].contiguous()


def frechet_truth64(X, A, B=None):
    """the float64 evaluation of the inputs as they are (already rounded to the dtype under test)"""
    return frechet_ref(X, A, B, torch.float64)


def series_frechet(X, A, B=None, terms=None):
    """the defining power series in float64: L = sum_k 1/k! sum_{i+j=k-1} X^i A X^j, and L2 the same with both
    orders of A and B between three powers.  `terms` powers of X are used: exact for a nilpotent X with
    terms >= D (the finite double sum)."""
    X, A = X.double(), A.double()
    D = X.shape[-1]
    terms = D if terms is None else terms
    pw = [torch.eye(D, dtype=torch.float64).expand_as(X)]
    for _ in range(1, terms):
        pw.append(pw[-1] @ X)
    fact = [1.0]
    for k in range(1, 3 * terms + 3):
        fact.append(fact[-1] * k)
    out = torch.zeros(torch.broadcast_shapes(X.shape, A.shape), dtype=torch.float64)
    if B is None:
        for i in range(terms):
            for j in range(terms):
                out = out + pw[i] @ A @ pw[j] / fact[i + j + 1]
        return out
    B = B.double()
    for i in range(terms):
        for j in range(terms):
            for l in range(terms):
                out = out + (pw[i] @ A @ pw[j] @ B @ pw[l] + pw[i] @ B @ pw[j] @ A @ pw[l]) / fact[i + j + l + 2]
    return out


# ------------------------------------------------------------------------------------------ the model
def lie_plan(X, max_order=10000, tol=1e-32, depth=0):
    """(s, m, r_m, r_prev) per record, in X's dtype, by the rules of nfm_lie_ops.hpp: s from frexp of ||X||_1 (column
    sums accumulated in order, as the kernel does), clamped to MAX_SQUARINGS; m the first n >= 2 whose term bound
    (||Y||_F^n / n!)^2 is <= D^2 tol, at most max_order; the derivative of depth `depth` runs `depth` degrees further
    (min(m + depth, max_order)), its terms lagging the exponential's by that many powers of Y.  r_m and r_prev are
    the ratios bound / limit at m and at m - 1 (before `depth` is added): a value within rounding of 1 marks a record
    whose degree a differently rounded ||Y||_F may move by one."""
    D = X.shape[-1]
    x = X.reshape(-1, D, D)
    n = x.shape[0]
    col = torch.zeros(n, D, dtype=X.dtype)
    for i in range(D):
        col = col + x[:, i, :].abs()
    nrm = col.amax(-1)
    finite = torch.isfinite(x).all(-1).all(-1)
    e = torch.frexp(torch.where(torch.isfinite(nrm), nrm, torch.ones_like(nrm)))[1].to(torch.int64)
    s = e.clamp(0, MAX_SQUARINGS)
    s = torch.where(torch.isfinite(nrm), s, torch.full_like(s, MAX_SQUARINGS))
    s = torch.where(finite, s, torch.zeros_like(s))
    y = x * torch.ldexp(torch.ones(n, dtype=X.dtype), -s.to(torch.int32))[:, None, None]
    ss = torch.zeros(n, dtype=X.dtype)
    for k in range(D * D):
        ss = ss + y.reshape(n, -1)[:, k] ** 2
    b = ss.double().sqrt()
    lim = float(D * D) * tol
    term = b.clone()
    m = torch.ones(n, dtype=torch.int64)
    r_m = torch.full((n,), float('inf'), dtype=torch.float64)
    r_prev = torch.full((n,), float('inf'), dtype=torch.float64)
    active = torch.ones(n, dtype=torch.bool)
    k = 2
    while k <= max_order and bool(active.any()):
        prev = term * term / lim if lim > 0 else torch.full_like(term, float('inf'))
        term = torch.where(active, term * b / k, term)
        m = torch.where(active, torch.full_like(m, k), m)
        ratio = term * term / lim if lim > 0 else torch.where(term > 0, torch.full_like(term, float('inf')), term)
        r_prev = torch.where(active, prev, r_prev)
        r_m = torch.where(active, ratio, r_m)
        stop = ~(term * term > lim) | ~(term < float('inf'))
        active = active & ~stop
        k += 1
    m = frechet_degree(m, depth, max_order)
    shape = X.shape[:-2]
    return s.reshape(shape), m.reshape(shape), r_m.reshape(shape), r_prev.reshape(shape)


def frechet_degree(m, depth, max_order):
    """the degree a derivative of depth `depth` runs to: min(m + depth, max_order), never below m"""
    if not depth:
        return m
    return torch.where(m + depth <= max_order, m + depth, m.clamp(min=min(max_order, 2 ** 31 - 1)))


def expm_model(X, dtype, max_order=10000, tol=1e-32, plan=None):
    """The forward part of `frechet_model`: E alone, Y = X / 2^s, Horner  P <- I + Y P / k  for k = m .. 1 with m from
    `lie_plan(..., depth=0)`, then s squarings.  Returns (E, (s, m)); `plan` = (s, m) pins both per record.  Order 1
    is the kernel's closed form exp(x), with the plan (0, 0)."""
    X = X.to(dtype)
    D = X.shape[-1]
    batch = X.shape[:-2]
    if D == 1:
        z = torch.zeros(batch, dtype=torch.int64)
        return torch.where(torch.isfinite(X), torch.exp(X), torch.full_like(X, float('nan'))), (z, z)
    x = X.reshape(-1, D, D)
    n = x.shape[0]
    if plan is None:
        s, m = lie_plan(x, max_order, tol, 0)[:2]
    else:
        s, m = (torch.as_tensor(t).expand(batch).reshape(-1) for t in plan[:2])
    finite = torch.isfinite(x).all(-1).all(-1)
    f = torch.ldexp(torch.ones(n, dtype=dtype), -s.to(torch.int32))[:, None, None]
    y = torch.where(finite[:, None, None], x * f, torch.full_like(x, float('nan')))
    eye = torch.eye(D, dtype=dtype).expand(n, D, D)
    e = eye.clone()
    for k in range(int(m.max()) if n else 0, 0, -1):
        rk = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(k), dtype=dtype)
        e = torch.where((m >= k)[:, None, None], eye + (y @ e) * rk, e)
    for q in range(int(s.max()) if n else 0):
        e = torch.where((s > q)[:, None, None], e @ e, e)
    return e.reshape(X.shape), (s.reshape(batch), m.reshape(batch))


def frechet_model(X, A, B, dtype, max_order=10000, tol=1e-32, plan=None, with_e=False):
    """The kernel's formulas in `dtype`, batched over equal batch shapes: Y = X / 2^s, A' = A / 2^s, B' = B / 2^s,
    Horner  H <- (A' P^B + B' P^A + Y H) / k,  P^B <- (B' P + Y P^B) / k,  P^A <- (A' P + Y P^A) / k,
    P <- I + Y P / k  for k = m .. 1, then s times  H <- H E + L^A L^B + L^B L^A + E H,  L <- L E + E L,  E <- E E.
    `plan` = (s, m) pins the squarings and the degree (per record); otherwise they come from `lie_plan` in `dtype`.
    Order 1 is the kernel's closed form exp(x) a (b).  `with_e` returns (derivative, E): the exponential the same
    recurrences carry (a non-finite direction makes it NaN too, as in the kernel)."""
    X, A = X.to(dtype), A.to(dtype)
    B = None if B is None else B.to(dtype)
    D = X.shape[-1]
    if D == 1:
        ex = torch.where(torch.isfinite(X), torch.exp(X), torch.full_like(X, float('nan')))
        out = ex * A if B is None else ex * A * B
        return (out, ex.expand_as(out)) if with_e else out
    shape = torch.broadcast_shapes(X.shape, A.shape, *(() if B is None else (B.shape,)))
    x = X.expand(shape).reshape(-1, D, D)
    a = A.expand(shape).reshape(-1, D, D)
    b = None if B is None else B.expand(shape).reshape(-1, D, D)
    n = x.shape[0]
    if plan is None:
        s, m = lie_plan(x, max_order, tol, 1 if b is None else 2)[:2]
    else:
        s, m = (torch.as_tensor(t).expand(shape[:-2]).reshape(-1) for t in plan[:2])
    finite = torch.isfinite(x).all(-1).all(-1) & torch.isfinite(a).all(-1).all(-1)
    if b is not None:
        finite = finite & torch.isfinite(b).all(-1).all(-1)
    f = torch.ldexp(torch.ones(n, dtype=dtype), -s.to(torch.int32))[:, None, None]
    y = torch.where(finite[:, None, None], x * f, torch.full_like(x, float('nan')))
    ap = a * f
    eye = torch.eye(D, dtype=dtype).expand(n, D, D)
    e, la = eye.clone(), torch.zeros_like(x)
    if b is not None:
        bp = b * f
        lb, h = torch.zeros_like(x), torch.zeros_like(x)
    for k in range(int(m.max()) if n else 0, 0, -1):
        on = (m >= k)[:, None, None]
        rk = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(k), dtype=dtype)
        if b is not None:
            h = torch.where(on, (ap @ lb + bp @ la + y @ h) * rk, h)
            lb = torch.where(on, (bp @ e + y @ lb) * rk, lb)
        la = torch.where(on, (ap @ e + y @ la) * rk, la)
        e = torch.where(on, eye + (y @ e) * rk, e)
    for q in range(int(s.max()) if n else 0):
        on = (s > q)[:, None, None]
        if b is not None:
            h = torch.where(on, (h @ e + la @ lb) + (lb @ la + e @ h), h)
            lb = torch.where(on, lb @ e + e @ lb, lb)
        la = torch.where(on, la @ e + e @ la, la)
        e = torch.where(on, e @ e, e)
    out = (la if b is None else h).reshape(shape)
    return (out, e.reshape(shape)) if with_e else out


# ------------------------------------------------------------------------------------------ measures and verdicts
def norm1(X):
    return X.double().abs().sum(-2).amax(-1)


def unit(X, dtype):
    """D eps (1 + ||X||_1) per record"""
    return X.shape[-1] * torch.finfo(dtype).eps * (1.0 + norm1(X.cpu()))


def err(K, T):
    """max|K - T| / max|T| per record, as test_gpu_lie.rel; a non-finite result counts as inf"""
    K, T = K.detach().cpu().double(), T.detach().cpu().double()
    d = (K - T).abs().amax((-2, -1))
    den = T.abs().amax((-2, -1))
    e = d / den
    e = torch.where((den == 0) & (d == 0), torch.zeros_like(e), e)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float('inf')))


def c_of(K, T, X, dtype):
    """error / unit per record"""
    return err(K, T) / unit(X, dtype).expand_as(err(K, T))


def c_bound(c_ref, D):
    """the constant a kernel is held to, from the worst constant of the reference on the same inputs.  Order 1 is
    held to the floor: there the block matrix is a 2 x 2 Jordan block, on which matrix_exp in float32 is up to 23
    units off (gen-2, 2000 records), so the reference sets no bar and may not widen one."""
    if D == 1:
        return C_FLOOR
    c_ref = float(c_ref)
    assert c_ref <= C_REF_CAP, f'C_ref = {c_ref:.2f} exceeds {C_REF_CAP}: not a usable class'
    return max(C_FLOOR, 2.0 * c_ref)


def verdict(c, cmax, label):
    """None when every record is within cmax units; otherwise a message that names the class, how many records
    failed, and the worst of them with error / unit"""
    c = c.reshape(-1)
    bad = torch.nonzero(~(c <= cmax)).reshape(-1)
    if bad.numel() == 0:
        return None
    w = int(bad[torch.argmax(c[bad])])
    return (f'{label}: {bad.numel()} of {c.numel()} records over {cmax:.2f} units; worst record {w} at '
            f'{float(c[w]):.2f} units; first records {bad[:8].tolist()}')


def held(K, T, X, dtype, cmax, label):
    msg = verdict(c_of(K, T, X, dtype), cmax, label)
    assert msg is None, msg


def class_verdicts(K, T, R, X, dtype, where, label, factor=1.0, show=False):
    """every class of a batch of classes held to factor * max(4, 2 C_ref), C_ref from the reference R on the same
    records; all failing classes are reported together"""
    D = X.shape[-1]
    ck, cr = c_of(K, T, X, dtype), c_of(R, T, X, dtype)
    msgs = []
    for cls, sl in where:
        cmax = factor * c_bound(cr[sl].max(), D)
        if show:
            print(f'{label} {cname(cls)}: kernel {float(ck[sl].max()):.2f} reference {float(cr[sl].max()):.2f} '
                  f'bound {cmax:.2f} units')
        msg = verdict(ck[sl], cmax, f'{label} {cname(cls)}')
        if msg:
            msgs.append(msg)
    assert not msgs, '\n'.join(msgs)


def truncated_verdict(K, X, A, B, dtype, max_order, tol, margin=1e-3):
    """error / unit per record of a result computed with `max_order` / `tol` against the model in float64, with the
    squarings and the degree pinned to what `dtype` arithmetic gives.  A record whose term bound is within `margin`
    of the limit may have taken the neighbouring degree: it gets the smaller of the two errors.  A None: the
    exponential itself (`expm_model`, depth 0)."""
    depth = 0 if A is None else (1 if B is None else 2)
    X = X.cpu().to(dtype)
    s, m, r_m, r_prev = lie_plan(X, max_order, tol)

    def at(mm):
        plan = (s, frechet_degree(mm, depth, max_order))
        if A is None:
            return c_of(K, expm_model(X, torch.float64, plan=plan)[0], X, dtype)
        return c_of(K, frechet_model(X, A.cpu(), None if B is None else B.cpu(), torch.float64, plan=plan), X, dtype)

    c = at(m)
    up = ((r_m - 1).abs() < margin) & (m < max_order)
    down = ((r_prev - 1).abs() < margin) & (m > 2)
    if bool(up.any()):
        c = torch.where(up, torch.minimum(c, at(m + 1)), c)
    if bool(down.any()):
        c = torch.where(down, torch.minimum(c, at(m - 1)), c)
    return c


# ------------------------------------------------------------------------------------------ the 40-digit fixture
@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, 'lie_frechet.npz'))


def fixture_classes():
    """(class, slice) in the order the fixture stores its records"""
    out, at = [], 0
    for cls in CLASSES:
        n = FIXTURE_COUNT[cls[0]]
        out.append((cls, slice(at, at + n)))
        at += n
    return out


def fixture_records(D):
    """(X, A, B, L, L2) of an order of the fixture, float64 tensors"""
    g = fixture()
    return tuple(torch.from_numpy(g[f'{k}_{D}']) for k in ('x', 'a', 'b', 'L', 'L2'))


@functools.lru_cache(maxsize=None)
def fixture_c_ref(D, depth):
    """{class: worst error / unit of the float64 block identities against the 40-digit truth}: the constant of the
    float64 reference, measured where a truth beyond float64 exists (orders 2..4)"""
    x, a, b, L, L2 = fixture_records(D)
    c = c_of(frechet_truth64(x, a, b if depth == 2 else None), L2 if depth == 2 else L, x, torch.float64)
    return {cls: float(c[sl].max()) for cls, sl in fixture_classes()}


# ------------------------------------------------------------------------------------------ the forward kernels
# Input classes, a conditioning unit and per-record verdicts for `ExpmOp` itself (test_gpu_lie_forward.py and
# test_lie_host.py).  The unit of the Frechet tests above, D eps (1 + ||X||_1), is not a conditioning bound: on general
# matrices of ||X||_1 = 80 a float32 transcription of the kernel's formulas is 4 of those units off and matrix_exp 100.
# The forward kernels are held to the Frobenius error ||K - T||_F / ||T||_F in units of D eps max(1, cond_exp(X)),
# cond_exp(X) = ||K(X)||_2 ||X||_F / ||e^X||_F, K(X) the D^2 x D^2 matrix of the Frechet derivative: the relative
# change of e^X that a relative perturbation eps of X can cause, which no algorithm can be asked to beat.
FWD_CLASSES = tuple(('gen', v) for v in (1e-3, 0.5, 8.0, 30.0, 60.0, 80.0)) + \
    (('skew', 200.0), ('skew', 1000.0), ('nilp', 5.0)) + \
    tuple(('shift', v) for v in (10.0, 40.0, 80.0)) + (('tri', 30.0), ('tri', 100.0)) + \
    tuple(('edge', v) for v in (1.0, 2.0, 4.0, 8.0))
FWD_CLASSES_F64 = FWD_CLASSES + (('shift', 300.0), ('gen', 300.0))     # float64 only: out of float32's range
FWD_FIXTURE_ORDERS = (2, 3, 4, 5, 6, 7)
FWD_FIXTURE_COUNT = 6                        # records per class and order in golden/lie_forward.npz
FWD_N = 768                                  # the interleaved batch of the GPU tests: 12 wavefronts (cond_exp of it
#                                              takes 0.5 s on the host at order 8)
FWD_N_CLASS = 2000                           # records per class of the host's larger draw at orders <= 3
SHIFT_NORM = 2.0                             # ||G||_1 of the shift classes, X = G - a I
EDGE_BITS = 12                               # the edge classes' entries are multiples of ||X||_1 / 2^12


# classes that miss the range condition (`in_range`) at an order, by their construction: e^X = e^-80 e^G, and max|e^G|
# with ||G||_1 = 2 is as low as e^-2 at order 1 and below 0.66 on 49%, 11% and 1.7% of 2000 records at orders 1, 2, 3,
# which puts max|e^X| under 2^10 tiny = 1.2e-35 in float32 (from order 4 on none of 2000 is; shift-40 covers 1..3)
FWD_UNUSABLE = {('f32', D): (('shift', 80.0),) for D in (1, 2, 3)}


def fwd_classes(dn, D):
    """the classes of a dtype that are usable at an order, in the order the interleaved batches cycle through"""
    out = FWD_CLASSES_F64 if dn == 'f64' else FWD_CLASSES
    return tuple(c for c in out if c not in FWD_UNUSABLE.get((dn, D), ()))


def build_fwd(cls, n, D, gen):
    """n float64 matrices of a forward class.  gen, skew, nilp: `build_x`.  shift-a: G - a I with ||G||_1 = 2, the
    exponential is e^-a e^G and every Horner step cancels.  tri-v: strictly upper part of 1-norm v, diagonal uniform
    in [-3, 0]: non-normal.  edge-p: ||X||_1 = p, a power of two, exactly -- entries cut to multiples of p / 2^12
    (every column sum is then exact in float32, in any order), the largest entry of the heaviest column raised by
    what the cut took."""
    kind, v = cls
    if kind in ('gen', 'skew', 'nilp'):
        return build_x(cls, n, D, gen)
    if kind == 'shift':
        return build_x(('gen', SHIFT_NORM), n, D, gen) - v * torch.eye(D, dtype=torch.float64)
    if kind == 'tri':
        up = build_x(('nilp', v), n, D, gen)
        return up + torch.diag_embed(-3.0 * torch.rand(n, D, dtype=torch.float64, generator=gen))
    assert kind == 'edge'
    q = v / 2.0 ** EDGE_BITS
    g = build_x(('gen', v), n, D, gen)
    g = torch.sign(g) * torch.floor(g.abs() / q) * q
    col = g.abs().sum(-2)
    j = col.argmax(-1)
    i = g.abs()[torch.arange(n), :, j].argmax(-1)
    sgn = torch.where(g[torch.arange(n), i, j] < 0, -1.0, 1.0)
    g[torch.arange(n), i, j] += sgn * (v - col[torch.arange(n), j])
    return g


@functools.lru_cache(maxsize=None)
def fwd_inputs(cls, n, D, dn, salt=0):
    """n records of a forward class, rounded to the dtype `dn`; shared, not to be written to"""
    return build_fwd(cls, n, D, _seed(cls, D, salt + 100)).to(DT[dn])


def fwd_class_index(n, dn, D):
    """the class of record i of an interleaved batch: i mod the number of classes, so that every wavefront holds
    every class, and with them every (s, m) from (0, 5) to (10, 22)"""
    return torch.arange(n) % len(fwd_classes(dn, D))


@functools.lru_cache(maxsize=None)
def fwd_batch(n, D, dn, salt=0):
    """(X, class index) of the interleaved batch of n records: record i is record i // C of class i mod C"""
    classes = fwd_classes(dn, D)
    C = len(classes)
    per = -(-n // C)
    X = torch.stack([fwd_inputs(cls, per, D, dn, salt) for cls in classes], 1).reshape(per * C, D, D)[:n]
    return X.contiguous(), fwd_class_index(n, dn, D)


def in_range(T, dtype):
    """the range condition of a usable record: 2^10 tiny <= max|e^X| <= 2^-10 max of the dtype: the entries that carry
    the Frobenius error are normal numbers with ten bits of room, so the relative bound means what it says"""
    fi = torch.finfo(dtype)
    big = T.double().abs().amax((-2, -1))
    return (big >= 2.0 ** 10 * fi.tiny) & (big <= 2.0 ** -10 * fi.max)


def cond_exp(X):
    """(cond_exp, ||e^X||_F) per record in float64: K(X) column by column from the block identity
    expm([[X, E_ij], [0, X]])[:D, D:] over the D^2 unit directions, in chunks of records; order 1: |x|"""
    X = X.double()
    D = X.shape[-1]
    x = X.reshape(-1, D, D)
    if D == 1:
        return x.abs().reshape(X.shape[:-2]), torch.exp(x).abs().reshape(X.shape[:-2])
    n = x.shape[0]
    dirs = torch.eye(D * D, dtype=torch.float64).reshape(D * D, D, D)
    cond, nrm = torch.empty(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64)
    step = max(1, 2 ** 21 // (4 * D ** 4))
    for at in range(0, n, step):
        xc = x[at:at + step]
        Z, (r, c) = _blocks(xc[:, None], dirs, None, torch.float64)
        Z = torch.linalg.matrix_exp(Z)
        K = Z[..., r, c].reshape(-1, D * D, D * D)                # row (i, j): vec L(X, E_ij) -- K transposed
        ef = torch.linalg.matrix_norm(Z[:, 0, :D, :D])
        cond[at:at + step] = torch.linalg.matrix_norm(K, 2) * torch.linalg.matrix_norm(xc) / ef
        nrm[at:at + step] = ef
    return cond.reshape(X.shape[:-2]), nrm.reshape(X.shape[:-2])


def fwd_unit(X, dtype, cond=None):
    """D eps max(1, cond_exp(X)) per record (`cond`: a cached cond_exp of the same records)"""
    cond = cond_exp(X.cpu())[0] if cond is None else cond
    return X.shape[-1] * torch.finfo(dtype).eps * cond.clamp(min=1.0)


def fwd_err(K, T):
    """||K - T||_F / ||T||_F per record; a non-finite result counts as inf"""
    K, T = K.detach().cpu().double(), T.detach().cpu().double()
    e = torch.linalg.matrix_norm(K - T) / torch.linalg.matrix_norm(T)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float('inf')))


def fwd_c(K, T, X, dtype, cond=None):
    """error / unit per record"""
    return fwd_err(K, T) / fwd_unit(X, dtype, cond)


def fwd_truth64(X):
    """matrix_exp in float64 on the inputs as they are (rounded to float32): the truth of float32 results, held to
    the 40-digit fixture by test_lie_host.py; order 1: exp"""
    X = X.cpu().double()
    return torch.exp(X) if X.shape[-1] == 1 else torch.linalg.matrix_exp(X)


@functools.lru_cache(maxsize=None)
def fwd_case(D, dn, salt=0):
    """(X, class index, truth, cond_exp) of the interleaved batch the GPU tests judge at an order: float32 the
    FWD_N-record draw with the float64 matrix_exp as truth, float64 the 40-digit fixture (orders 2..7; order 1: the
    draw, exp in float64 is correctly rounded to an ulp).  The range condition is asserted on every record."""
    if dn == 'f64' and D > 1:
        X, T = fwd_fixture_records(D)
        idx = fwd_class_index(X.shape[0], dn, D)
    else:
        X, idx = fwd_batch(FWD_N, D, dn, salt)
        T = fwd_truth64(X)
    ok = in_range(T, DT[dn])
    assert bool(ok.all()), f'{dn} D={D}: records {torch.nonzero(~ok).reshape(-1)[:8].tolist()} out of range'
    return X, idx, T, cond_exp(X)[0]


def fwd_worst(c, idx, classes):
    """{class name: worst value} of a per-record measure of an interleaved batch"""
    return {cname(cls): float(c[idx == q].max()) for q, cls in enumerate(classes) if bool((idx == q).any())}


def fwd_verdicts(c, idx, classes, cmax, label):
    """every class of an interleaved batch held to cmax units; all failing classes are reported together"""
    msgs = []
    for q, cls in enumerate(classes):
        rec = torch.nonzero(idx == q).reshape(-1)
        bad = rec[~(c[rec] <= cmax)]
        if bad.numel():
            w = int(bad[torch.argmax(c[bad])])
            msgs.append(f'{label} {cname(cls)}: {bad.numel()} of {rec.numel()} records over {cmax:.2f} units; worst '
                        f'record {w} at {float(c[w]):.2f} units; first records {bad[:8].tolist()}')
    assert not msgs, '\n'.join(msgs)


@functools.lru_cache(maxsize=None)
def fwd_fixture():
    return np.load(os.path.join(GOLDEN, 'lie_forward.npz'))


def fwd_fixture_records(D):
    """(X, e^X at 40 digits) of an order of the forward fixture, float64, interleaved by class"""
    g = fwd_fixture()
    return torch.from_numpy(g[f'x_{D}']), torch.from_numpy(g[f't_{D}'])
