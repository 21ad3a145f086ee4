"""Hard inputs, high-precision truths and per-record bounds of the solver accuracy tests (shared by
test_solver_accuracy_host.py and test_gpu_solver_accuracy.py).

Every measure returns ONE NUMBER PER RECORD: the batches carry a different power of two per record, so a batch
max-norm means nothing, and a wrong record with small entries cannot hide behind a large neighbour.

High precision (`hp`): float64 for float32 results, numpy.longdouble (64-bit mantissa, asserted) for float64
results.  A residual or a truth of order M then carries a rounding error of about M 2^-53 (M 2^-64) relative to
the scale it is compared on, against bounds of at least M 2^-23 (M 2^-52): below 1/16 of the bound with room.

Bounds, eps the machine epsilon of the dtype under test (none of them a new number):
  solves, M >= 5      eta_i <= 2 eta_oracle,i + 4 M eps, eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf): the
                      error model of conftest.py (`model_bound`, c = 4) applied to every record.
  inverses, dets      err_i <= 2 err_oracle,i + M eps (1 + cond_i / 8), max-norm relative error of the record
  M >= 5              against its own truth, cond_i = |A|_inf |A^-1|_inf: the per-matrix model of
                      test_gpu_large_orders.py::test_general_large_orders.
  A inv = I           max |A inv - I| <= 4 M . M eps (1 + cond_i / 8): the same test's residual bound (batchinv);
                      the symmetric inverses: <= |A|_inf max |A^-1| times the inverse's own bound above
                      (`identity_model_excess`: the oracle's residual there is of order eps cond^2).
  orders 1..4         closed forms, not backward stable: bit equality with the oracle (NaN positions included),
                      on graded families up to CLOSED_COND_MAX, where the oracle's results are all finite.
"""
import functools
import numpy as np
from conftest import EPS
from _dense_ref import NP, pairs, to_full, to_compact

HP = {'f32': np.float64, 'f64': np.longdouble}
ORDERS = tuple(range(1, 17))
NS = (209, 17)                    # three wavefronts + one full group of 16 + one record; one group + one record
CONDS = {'f32': (1e1, 1e3, 1e5), 'f64': (1e1, 1e6, 1e12)}
CLOSED_COND_MAX = {'f32': 1e3, 'f64': 1e6}       # orders <= 4: the oracle is finite for every record up to here
MIXED_COND = {'f32': 1e3, 'f64': 1e6}            # the positive definite records of the mixed batches
# exponents of the per-record powers of two.  Solves and inverses at M >= 5 carry 2^-k; closed forms and
# determinants carry 2^(k M): |k| M <= KM_MAX (narrowed for the determinants, which are small to begin with)
KMAX_LINEAR = {'f32': 40, 'f64': 400}
KM_MAX = {'f32': 96, 'f64': 900}
KM_MAX_DET = {'f32': 40, 'f64': 640}
BARELY_C = (0.25, 1.0, 4.0)
# the default batchinv / batchdet of order 3 (an adjugate) meet the LU-based bounds up to cond 1e2 (measured on an
# MI355X: 0.43 of them there, 1.5 times them at 1e3): of the graded conds, 1e1 is the one they are held to
ADJUGATE3_COND_MAX = 1e1


def barely_cs(M):
    """c of the barely definite family: 0.25, 1, 4, and two values M^2 below -- the last pivot of a factorisation is
    1 / (A^-1)_MM, about M lam_min for a random basis, and only comes down to the rounding level (eps a_MM) there"""
    return (0.25 / (M * M), 1.0 / (M * M)) + BARELY_C


def hp_ok():
    return np.finfo(np.longdouble).eps <= 2.0 ** -63


def cond_list(M, dn):
    """the graded conds an order is tested at (closed forms: up to the finite-oracle cond)"""
    return tuple(c for c in CONDS[dn] if M >= 5 or c <= CLOSED_COND_MAX[dn])


def kmax_closed(M, dn, det=False):
    return (KM_MAX_DET if det else KM_MAX)[dn] // M


def kmax_for(op, M, dn):
    """largest |k| of a per-record scale 2^k at which op's scaled result stays a normal number (asserted by
    test_solver_accuracy_host.py on the inputs themselves)"""
    if op in ('sym_det', 'batchdet'):
        return kmax_closed(M, dn, det=True)
    if M <= 4 and op == 'sym_solve':
        return KM_MAX[dn] // (M + 1)          # the right-hand side carries a power of two of its own
    if M <= 4 and op != 'batchmatvec':
        return kmax_closed(M, dn)
    return KMAX_LINEAR[dn]


# ------------------------------------------------------------------------------------------ builders
def _orth(rng, n, M):
    return np.linalg.qr(rng.standard_normal((n, M, M)))[0]


def _graded(M, cond):
    return np.logspace(0.0, -np.log10(cond), M) if M > 1 else np.ones(1)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def spd_graded(n, M, cond, dn, seed):
    """compact Q diag(lam) Q^T, lam log-spaced from 1 to 1 / cond, built in float64, symmetrised and rounded to
    the dtype; and a right-hand side.  Conds at which the rounding could cost definiteness are refused."""
    if cond * M * EPS[dn] >= 0.25:
        raise ValueError(f'cond {cond:g} at order {M} does not survive rounding to {dn}')
    rng = np.random.default_rng(seed)
    Q = _orth(rng, n, M)
    A = np.einsum('nij,j,nkj->nik', Q, _graded(M, cond), Q)
    A = (A + A.transpose(0, 2, 1)) / 2
    return _frozen(to_compact(A).astype(NP[dn]), rng.standard_normal((n, M)).astype(NP[dn]))


@functools.lru_cache(maxsize=None)
def general_graded(n, N, cond, dn, seed):
    """U diag(sigma) V^T, sigma log-spaced from 1 to 1 / cond, rounded to the dtype; and a vector"""
    rng = np.random.default_rng(seed)
    U, V = _orth(rng, n, N), _orth(rng, n, N)
    A = np.einsum('nij,j,nkj->nik', U, _graded(N, cond), V)
    return _frozen(A.astype(NP[dn]), rng.standard_normal((n, N)).astype(NP[dn]))


@functools.lru_cache(maxsize=None)
def pow2_scales(n, kmax, seed):
    """integer exponents in [-kmax, kmax], a different one per record as far as the range allows, both ends
    of the range present"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-kmax, kmax + 1, n)
    if n >= 2:
        k[rng.permutation(n)[:2]] = (-kmax, kmax)
    return _frozen(k.astype(np.int64))


def scaled(x, k):
    """x_i 2^(k_i), exact (ldexp), in x's dtype; k per record"""
    k = np.asarray(k).reshape((-1,) + (1,) * (x.ndim - 1))
    return np.ldexp(x, k).astype(x.dtype)


def is_normal(x, dn):
    """every value a normal number of the dtype (zeros excluded too)"""
    a = np.abs(np.asarray(x, np.float64 if dn == 'f32' else np.longdouble))
    fi = np.finfo(NP[dn])
    return bool(np.all((a >= fi.tiny) & (a <= fi.max)))


@functools.lru_cache(maxsize=None)
def barely_definite(n, M, c, dn, seed):
    """compact matrices that are positive definite before rounding, lam_min = c M eps lam_max (the other
    eigenvalues log-spaced between), built in high precision and rounded to the dtype: the last pivot of an
    unpivoted factorisation in the dtype is a tiny positive or a negative number, depending on rounding"""
    assert hp_ok()
    rng = np.random.default_rng(seed)
    Q = _orth(rng, n, M).astype(np.longdouble)
    lam = _graded(M, 1.0 / (c * M * EPS[dn])).astype(np.longdouble)
    A = np.einsum('nij,j,nkj->nik', Q, lam, Q)        # a congruence: definite whatever Q's own rounding
    A = (A + A.transpose(0, 2, 1)) / 2
    mat = np.stack([A[:, i, j] for i, j in pairs(M)], -1).astype(NP[dn])
    return _frozen(mat, rng.standard_normal((n, M)).astype(NP[dn]))


def fail_positions(n):
    """record 0, the last of a group, the first of the next, both sides of a wavefront boundary, the first
    record of the ragged last group and the very last record"""
    last_group = (n - 1) // 16 * 16
    return tuple(sorted({p for p in (0, 15, 16, 63, 64, last_group, n - 1) if p < n}))


def indefinite(npos, M, dn, seed):
    """well conditioned indefinite compact matrices (eigenvalues +-[1, 2], never definite, random basis)"""
    rng = np.random.default_rng(seed)
    Q = _orth(rng, npos, M)
    lam = rng.uniform(1, 2, (npos, M)) * np.where(rng.random((npos, M)) < 0.5, -1.0, 1.0)
    lam[:, 0] = -np.abs(lam[:, 0])
    if M > 1:
        lam[:, 1] = np.abs(lam[:, 1])
    A = np.einsum('nij,nj,nkj->nik', Q, lam, Q)
    return to_compact((A + A.transpose(0, 2, 1)) / 2).astype(NP[dn])


@functools.lru_cache(maxsize=None)
def mixed_sym(n, M, dn, seed, positions=None, kmax=None):
    """positive definite compact records at MIXED_COND with indefinite ones at `positions` (default
    `fail_positions(n)`), every record times its own power of two; (mat, vec, positions)"""
    pos = np.array(fail_positions(n) if positions is None else positions)
    mat, vec = spd_graded(n, M, MIXED_COND[dn], dn, seed)
    mat = mat.copy()
    mat[pos] = indefinite(len(pos), M, dn, seed + 1)
    k = pow2_scales(n, KMAX_LINEAR[dn] if kmax is None else kmax, seed + 2)
    return _frozen(scaled(mat, k), vec.copy(), pos)


@functools.lru_cache(maxsize=None)
def mixed_general(n, N, dn, seed, kind, positions=None, kmax=None):
    """general records whose diagonal serves as pivot throughout (positive definite at MIXED_COND, full storage)
    with failing ones at `positions`, made from 0.1 N(0, 1) + I: kind 'reversed' = its rows reversed, 'late' = the
    diagonal is fine until the last step that has a column to compare with (a unit pivot over an entry of 16: beyond
    the factor 8 that the diagonal-first attempt accepts); every record times its own power of two"""
    pos = np.array(fail_positions(n) if positions is None else positions)
    rng = np.random.default_rng(seed + 3)
    a = to_full(spd_graded(n, N, MIXED_COND[dn], dn, seed)[0])
    odd = rng.standard_normal((len(pos), N, N)) * 0.1 + np.eye(N)
    if kind == 'reversed':
        a[pos] = odd[:, ::-1]
    else:
        odd[:, N - 1, N - 2] = 16
        a[pos] = odd
    k = pow2_scales(n, KMAX_LINEAR[dn] if kmax is None else kmax, seed + 2)
    return _frozen(scaled(a.astype(NP[dn]), k), pos)


# ------------------------------------------------------------------------------------------ what a kernel sees
def ldl_pivots(mat, dn):
    """pivots of the unpivoted U^T D U factorisation of compact records, every operation rounded to the dtype
    (float32: products and sums formed in float64 and rounded once, which is what a fused multiply-add gives up
    to double rounding): which records an unpivoted first attempt accepts, d > 0 throughout"""
    T = NP[dn]
    a = to_full(mat).astype(np.float64)
    n, M, _ = a.shape
    piv = np.empty((n, M))
    rnd = (lambda x: x.astype(T).astype(np.float64))
    with np.errstate(all='ignore'):
        for k in range(M):
            d = a[:, k, k]
            piv[:, k] = d
            r = rnd(1.0 / d)
            for i in range(k + 1, M):
                u = rnd(a[:, k, i] * r)
                a[:, i, i:] = rnd(a[:, i, i:] - u[:, None] * a[:, k, i:])
    return piv


def diagonal_pivots_ok(a):
    """per record: does elimination without exchanges (float64) keep every diagonal pivot within a factor 8 of its
    column's maximum -- the rule by which batchinv / batchdet accept the diagonal at orders 9..16"""
    a = np.array(a, np.float64)
    n, N, _ = a.shape
    ok = np.ones(n, bool)
    with np.errstate(all='ignore'):
        for k in range(N):
            cmax = np.abs(a[:, k + 1:, k]).max(-1) if k + 1 < N else np.zeros(n)
            d = np.abs(a[:, k, k])
            ok &= (d >= 0.125 * cmax) & (d > 0)
            l = a[:, k + 1:, k] / a[:, k, k][:, None]
            a[:, k + 1:, k + 1:] -= l[:, :, None] * a[:, k, None, k + 1:]
    return ok


# ------------------------------------------------------------------------------------------ high precision
def hp_full(mat, dn):
    """compact records -> full symmetric, high precision"""
    mat = np.asarray(mat)
    M = int((np.sqrt(1 + 8 * mat.shape[-1]) - 1) // 2)
    f = np.empty(mat.shape[:-1] + (M, M), HP[dn])
    for c, (i, j) in enumerate(pairs(M)):
        f[..., i, j] = f[..., j, i] = mat[..., c]
    return f


def hp_compact(f):
    return np.stack([f[..., i, j] for i, j in pairs(f.shape[-1])], -1)


def hp_inv_det(a, dn):
    """inverse and determinant of every record by Gauss-Jordan with partial pivoting in high precision.  Every
    record is first scaled by a power of two to max |a| in [1, 2) (exact) so that no intermediate of a 16-fold
    product of scaled pivots leaves the range; the determinant is returned as (mantissa-like value, exponent):
    det_i = det[i] * 2^(dexp[i])."""
    if dn == 'f64':
        assert hp_ok()
    a = np.array(a, HP[dn])
    n, N, _ = a.shape
    e = np.frexp(np.abs(a).reshape(n, -1).max(-1))[1] - 1
    a = np.ldexp(a, -e[:, None, None])
    inv = np.broadcast_to(np.eye(N, dtype=HP[dn]), a.shape).copy()
    det = np.ones(n, HP[dn])
    rows = np.arange(n)
    with np.errstate(all='ignore'):
        for k in range(N):
            p = k + np.abs(a[:, k:, k]).argmax(-1)
            swap = p != k
            for m in (a, inv):
                tmp = m[rows, k].copy()
                m[rows, k] = m[rows, p]
                m[rows, p] = tmp
            det = np.where(swap, -det, det) * a[:, k, k]
            piv = a[:, k, k].copy()
            a[:, k] /= piv[:, None]
            inv[:, k] /= piv[:, None]
            f = a[:, :, k].copy()
            f[:, k] = 0
            inv -= f[:, :, None] * inv[:, k, None, :]
            a -= f[:, :, None] * a[:, k, None, :]
    return np.ldexp(inv, -e[:, None, None]), det, e * N


def hp_det_value(det, dexp):
    """the determinant as one high-precision number (the caller knows it is in range)"""
    return np.ldexp(det, dexp)


def _norm_inf(a):
    return np.abs(a).sum(-1).max(-1)


def cond_inf(a, dn, inv=None):
    """|A|_inf |A^-1|_inf per record (full matrices)"""
    a = np.asarray(a, HP[dn])
    inv = hp_inv_det(a, dn)[0] if inv is None else inv
    return (_norm_inf(a) * _norm_inf(inv)).astype(np.float64)


def solve_eta(a, x, b, dn):
    """normwise backward error of every record: |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), in high precision;
    a non-finite x counts as inf"""
    a, x, b = np.asarray(a, HP[dn]), np.asarray(x, HP[dn]), np.asarray(b, HP[dn])
    with np.errstate(all='ignore'):
        r = np.abs(b - np.einsum('nij,nj->ni', a, x)).max(-1)
        den = _norm_inf(a) * np.abs(x).max(-1) + np.abs(b).max(-1)
        eta = (r / den).astype(np.float64)
    return np.where(np.isfinite(eta), eta, np.inf)


def per_matrix_err(x, truth):
    """max-norm relative error of every matrix of the batch against its own truth"""
    x, truth = x.astype(np.float64).reshape(len(x), -1), truth.astype(np.float64).reshape(len(truth), -1)
    return np.abs(x - truth).max(-1) / np.maximum(np.abs(truth).max(-1), 1e-300)


def inv_err(got, truth, dn):
    """`per_matrix_err` in high precision (the per-record scales reach beyond float64's range of squares, not
    beyond its range: no 1e-300 guard is needed, a zero truth does not occur); non-finite results count as inf"""
    got, truth = np.asarray(got, HP[dn]).reshape(len(got), -1), np.asarray(truth, HP[dn]).reshape(len(truth), -1)
    with np.errstate(all='ignore'):
        e = (np.abs(got - truth).max(-1) / np.abs(truth).max(-1)).astype(np.float64)
    return np.where(np.isfinite(e), e, np.inf)


def det_err(got, det, dexp, dn):
    """|got - det| / |det| per record, the truth given as det 2^dexp (hp_inv_det)"""
    got = np.asarray(got, HP[dn])
    with np.errstate(all='ignore'):
        e = np.abs(np.ldexp(got, -dexp) / det - 1).astype(np.float64)
    return np.where(np.isfinite(e), e, np.inf)


def identity_residual(a, inv, dn):
    """max |A inv - I| per record, high precision"""
    a, inv = np.asarray(a, HP[dn]), np.asarray(inv, HP[dn])
    with np.errstate(all='ignore'):
        r = np.abs(np.einsum('nij,njk->nik', a, inv) - np.eye(a.shape[-1])).reshape(len(a), -1).max(-1)
    r = r.astype(np.float64)
    return np.where(np.isfinite(r), r, np.inf)


# ------------------------------------------------------------------------------------------ bounds
def eta_bound(eta_oracle, M, dn):
    return 2.0 * eta_oracle + 4.0 * M * EPS[dn]


def model_floor(M, dn, cond):
    return M * EPS[dn] * (1.0 + cond / 8.0)


def model_bound_rec(err_oracle, M, dn, cond):
    return 2.0 * err_oracle + model_floor(M, dn, cond)


def identity_bound(M, dn, cond):
    return 4.0 * M * model_floor(M, dn, cond)


def same_bits(x, y):
    """NaN positions equal, every other value equal (signed zeros compare equal, as in the existing tests)"""
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and bool(((x == y) | (np.isnan(x) & np.isnan(y))).all())


def worst(ratio):
    """(largest value, index of its record) of a per-record ratio"""
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


# ------------------------------------------------------------------------------------------ excess = measure / bound
class Truth:
    """high-precision full matrices, inverses, determinants (det 2^dexp) and cond_inf of a batch, computed once"""

    def __init__(self, a_full, dn):
        self.dn = dn
        self.a = np.asarray(a_full, HP[dn])
        self.n, self.M = self.a.shape[:2]
        self.inv, self.det, self.dexp = hp_inv_det(self.a, dn)
        self.cond = cond_inf(self.a, dn, self.inv)


def sym_truth(mat, dn):
    return Truth(hp_full(mat, dn), dn)


def solve_excess(got, ref, tr, vec):
    """eta_i / (2 eta_ref,i + 4 M eps) per record: <= 1 passes"""
    return solve_eta(tr.a, got, vec, tr.dn) / eta_bound(solve_eta(tr.a, ref, vec, tr.dn), tr.M, tr.dn)


def inv_excess(got, ref, tr, diag=False):
    """err_i / (2 err_ref,i + M eps (1 + cond_i / 8)) per record; full (n, M, M) results, or the diagonals (n, M)"""
    truth = np.diagonal(tr.inv, axis1=1, axis2=2) if diag else tr.inv
    return inv_err(got, truth, tr.dn) / model_bound_rec(inv_err(ref, truth, tr.dn), tr.M, tr.dn, tr.cond)


def det_excess(got, ref, tr):
    return det_err(got, tr.det, tr.dexp, tr.dn) / model_bound_rec(det_err(ref, tr.det, tr.dexp, tr.dn), tr.M, tr.dn, tr.cond)


def identity_excess(got, tr):
    """max |A inv - I| / (4 M . M eps (1 + cond_i / 8)) per record"""
    return identity_residual(tr.a, got, tr.dn) / identity_bound(tr.M, tr.dn, tr.cond)


def identity_model_excess(got, ref, tr):
    """the symmetric inverses, whose reference does not meet the plain A inv = I bound (one triangle of an inverse
    has a residual of order eps cond^2, whoever computes it): max |A inv - I| over what the per-matrix model of the
    inverse allows it to be.  inv = truth + d with max |d| <= (2 err_ref,i + M eps (1 + cond_i / 8)) max |truth|
    gives max |A inv - I| = max |A d| <= |A|_inf max |d|: a triangle inequality, nothing measured.  The residual
    is formed from A and the result alone, in high precision."""
    allowed = _norm_inf(tr.a).astype(np.float64) * np.abs(tr.inv).reshape(tr.n, -1).max(-1).astype(np.float64) * \
        model_bound_rec(inv_err(ref, tr.inv, tr.dn), tr.M, tr.dn, tr.cond)
    return identity_residual(tr.a, got, tr.dn) / allowed


def matvec_excess(got, a, v, dn):
    """batchmatvec: |got - A v| / (N eps |A| |v|) per component, the worst of each record (an N-term sum of
    products each rounded once: (1 + eps/2)^(N+1) - 1 < N eps for N >= 2; N = 1: one rounding, eps / 2)"""
    a, v = np.asarray(a, HP[dn]), np.asarray(v, HP[dn])
    N = a.shape[-1]
    truth = np.einsum('nij,nj->ni', a, v)
    scale = np.einsum('nij,nj->ni', np.abs(a), np.abs(v))
    with np.errstate(all='ignore'):
        e = (np.abs(np.asarray(got, HP[dn]) - truth) / (N * EPS[dn] * scale)).astype(np.float64)
    return np.where(np.isfinite(e), e, np.inf).max(-1)


# ------------------------------------------------------------------------------------------ the second-launch case
BIG_N = (1 << 20) + 1
BIG_EVERY = 4099
BIG_BASE = 4093            # the big batch repeats a base of this many records (a prime, coprime to 16 and BIG_EVERY)


def big_fail_positions():
    return np.unique(np.r_[np.arange(0, BIG_N, BIG_EVERY), BIG_N - 1])


def big_selection():
    """both ends of the batch, the first 40 marked groups and the groups on either side of each (the selection
    of test_large_batches_redo_marked_groups_in_a_second_launch), and the last marked group's surroundings"""
    bad = big_fail_positions()
    near = [np.arange(max(b // 16 * 16 - 16, 0), min(b // 16 * 16 + 32, BIG_N)) for b in np.r_[bad[:40], bad[-2:]]]
    return np.unique(np.concatenate([np.arange(0, 600), np.arange(BIG_N - 300, BIG_N)] + near))


def big_tile(base, k):
    """record i of the big batch = base[i mod BIG_BASE] 2^(k_i)"""
    return scaled(base[np.arange(BIG_N) % BIG_BASE], k)
