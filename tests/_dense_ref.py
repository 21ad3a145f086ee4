"""Dense float64 references, seeded inputs and derived bounds of the compact-storage structure tests
(shared by test_structure_host.py, test_gpu_sym_structure.py and test_gpu_autograd_shapes.py).

Compact storage is the diagonal first, then the rows of the upper triangle (`sym.py`): `pairs(M)` lists the
(i, j) of every stored entry in that order.

Bounds, per component, eps the machine epsilon of the dtype under test (2^-23 / 2^-52):
  sym_matmul   |got - truth| <= (T + 4) eps S.  truth = J^T H J in float64 on the same inputs (J H J^T where
               the oracle evaluates that: compact H with k == d in {2, 3}, quirk Q16), S the same product of
               |J| and |H|, T the number of accumulated terms: k (k + 1) / 2 for compact H (k squares and
               k (k - 1) / 2 cross terms), k for diagonal H.  A T-term sum whose terms each take at most four
               roundings: (1 + eps/2)^(T + 4) - 1 < (T + 4) eps, nothing tuned.
  sym_outer2   out_ii = x_i y_i, out_ij = x_i y_j + x_j y_i: two products and one sum, so
               |got - truth| <= 2 eps (|x_i y_j| + |x_j y_i|)  (diagonal: 2 eps |x_i y_i|).
"""
import functools
import numpy as np

EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
NP = {'f32': np.float32, 'f64': np.float64}
NS = (1, 63, 65, 257, 1573)          # wave, 256-lane tile, 3 * 512 + 37: a ragged tail at each
ORDERS = tuple(range(1, 17))
KD = (1, 2, 3, 4, 5, 8, 9, 16)       # sym_matmul grid; anything beyond 4 runs the big-order kernel
EIG_GAP = 0.1


def pairs(M):
    return [(i, i) for i in range(M)] + [(i, j) for i in range(M) for j in range(i + 1, M)]


def order_of(K):
    M = int((np.sqrt(1 + 8 * K) - 1) // 2)
    assert M * (M + 1) // 2 == K, K
    return M


def to_full(c):
    """compact (..., K) -> full symmetric (..., M, M), float64"""
    c = np.asarray(c, np.float64)
    M = order_of(c.shape[-1])
    f = np.empty(c.shape[:-1] + (M, M))
    for k, (i, j) in enumerate(pairs(M)):
        f[..., i, j] = f[..., j, i] = c[..., k]
    return f


def to_compact(f):
    """full (..., M, M) -> compact (..., K) from the upper triangle, float64"""
    f = np.asarray(f, np.float64)
    return np.stack([f[..., i, j] for i, j in pairs(f.shape[-1])], -1)


def spd_np(n, M, dtype, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, M, M))
    A = G @ G.transpose(0, 2, 1) / M + np.eye(M)
    iu = [(i, j) for i in range(M) for j in range(i + 1, M)]
    c = np.concatenate([np.stack([A[:, i, i] for i in range(M)], -1)] +
                       ([np.stack([A[:, i, j] for i, j in iu], -1)] if iu else []), -1)
    return c.astype(dtype), rng.standard_normal((n, M)).astype(dtype)


# ---------------------------------------------------------------------------------- sym_matmul
@functools.lru_cache(maxsize=None)
def matmul_inputs(n, k, d, dn, diag):
    """seeded jacobians (n, k, d) and hessians (n, k (k + 1) / 2), or their diagonals (n, k)"""
    rng = np.random.default_rng(7000 + 97 * k + 13 * d + n)
    j = rng.standard_normal((n, k, d)).astype(NP[dn])
    h, _ = spd_np(n, k, NP[dn], 8000 + 31 * k + d + n)
    if diag:
        h = np.ascontiguousarray(h[:, :k])
    j.setflags(write=False)
    h.setflags(write=False)
    return j, h


def matmul_is_diag(k, h):
    """how the oracle and the facade read `h`: (n, 1) at k == 1 is the compact reading"""
    return h.shape[-1] == k and k != 1


def matmul_flips(k, d, diag):
    """quirk Q16: the reference's kernels for a compact hessian and k == d in {2, 3} evaluate J H J^T"""
    return (not diag) and k == d and k in (2, 3)


def matmul_truth(j, h):
    """(truth, S, T) of the module comment, float64, compact (n, d (d + 1) / 2)"""
    j = np.asarray(j, np.float64)
    h = np.asarray(h, np.float64)
    k, d = j.shape[-2:]
    diag = matmul_is_diag(k, h)

    def full(x):
        if not diag:
            return to_full(x)
        f = np.zeros(x.shape[:-1] + (k, k))
        f[..., np.arange(k), np.arange(k)] = x
        return f

    def prod(J, H):
        if matmul_flips(k, d, diag):
            return J @ H @ np.swapaxes(J, -1, -2)
        return np.swapaxes(J, -1, -2) @ H @ J
    truth = to_compact(prod(j, full(h)))
    S = to_compact(prod(np.abs(j), full(np.abs(h))))
    return truth, S, (k if diag else k * (k + 1) // 2)


def matmul_excess(got, j, h, dn):
    """max over components of |got - truth| / ((T + 4) eps S): <= 1 passes"""
    truth, S, T = matmul_truth(j, h)
    err = np.abs(np.asarray(got, np.float64) - truth)
    bound = (T + 4) * EPS[dn] * S
    ok = bound > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------- sym_outer2
@functools.lru_cache(maxsize=None)
def outer2_inputs(n, M, dn):
    rng = np.random.default_rng(9000 + 17 * M + n)
    x = rng.standard_normal((n, M)).astype(NP[dn])
    y = rng.standard_normal((n, M)).astype(NP[dn])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def outer2_truth(x, y):
    """(truth, scale): out_ii = x_i y_i, out_ij = x_i y_j + x_j y_i; scale the same with absolute values"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    M = x.shape[-1]
    t, s = [], []
    for i, j in pairs(M):
        a, b = x[..., i] * y[..., j], x[..., j] * y[..., i]
        t.append(a if i == j else a + b)
        s.append(np.abs(a) if i == j else np.abs(a) + np.abs(b))
    return np.stack(t, -1), np.stack(s, -1)


def outer2_formula(x, y, neg=False):
    """the same formula evaluated in the operands' own dtype (what a correct kernel computes)"""
    M = x.shape[-1]
    out = np.stack([x[..., i] * y[..., j] if i == j else x[..., i] * y[..., j] + x[..., j] * y[..., i]
                    for i, j in pairs(M)], -1)
    return -out if neg else out


def outer2_excess(got, x, y, dn, neg=False):
    """max over components of |got - truth| / (2 eps scale): <= 1 passes"""
    truth, scale = outer2_truth(x, y)
    err = np.abs(np.asarray(got, np.float64) - (-truth if neg else truth))
    bound = 2 * EPS[dn] * scale
    ok = bound > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------- eig_sym inputs
@functools.lru_cache(maxsize=None)
def eig_inputs(nb, n, seed):
    """symmetric Q diag(lam) Q^T (float64) whose eigenvalues are at least EIG_GAP apart, and lam (ascending):
    the F = 1 / (d_j - d_i) term of the eigenvector gradient then has a usable float32 reference"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((nb, n, n)))
    lam = rng.uniform(-1, 1, (nb, 1)) + np.cumsum(EIG_GAP + rng.uniform(0, 0.5, (nb, n)), -1)
    a = np.einsum('bij,bj,bkj->bik', Q, lam, Q)
    a = (a + a.transpose(0, 2, 1)) / 2
    a.setflags(write=False)
    return a, lam


def eig_gap(a):
    """smallest distance between two eigenvalues of any matrix of the batch (inf at order 1)"""
    w = np.linalg.eigvalsh(np.asarray(a, np.float64))
    return float(np.diff(w, axis=-1).min()) if w.shape[-1] > 1 else float('inf')
