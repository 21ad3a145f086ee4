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
    kinds = {'gen': 1, 'skew': 2, 'nilp': 3}
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


def frechet_model(X, A, B, dtype, max_order=10000, tol=1e-32, plan=None):
    """The kernel's formulas in `dtype`, batched over equal batch shapes: Y = X / 2^s, A' = A / 2^s, B' = B / 2^s,
    Horner  H <- (A' P^B + B' P^A + Y H) / k,  P^B <- (B' P + Y P^B) / k,  P^A <- (A' P + Y P^A) / k,
    P <- I + Y P / k  for k = m .. 1, then s times  H <- H E + L^A L^B + L^B L^A + E H,  L <- L E + E L,  E <- E E.
    `plan` = (s, m) pins the squarings and the degree (per record); otherwise they come from `lie_plan` in `dtype`.
    Order 1 is the kernel's closed form exp(x) a (b)."""
    X, A = X.to(dtype), A.to(dtype)
    B = None if B is None else B.to(dtype)
    D = X.shape[-1]
    if D == 1:
        ex = torch.where(torch.isfinite(X), torch.exp(X), torch.full_like(X, float('nan')))
        return ex * A if B is None else ex * A * B
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
    return (la if b is None else h).reshape(shape)


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
    of the limit may have taken the neighbouring degree: it gets the smaller of the two errors."""
    depth = 1 if B is None else 2
    X = X.cpu().to(dtype)
    s, m, r_m, r_prev = lie_plan(X, max_order, tol)

    def at(mm):
        plan = (s, frechet_degree(mm, depth, max_order))
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
