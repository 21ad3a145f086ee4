"""Inputs, truths and bounds shared by tests/test_svd_host.py and tests/test_gpu_svd.py (the Jacobi SVD solves of
`sugar`: method 'svd' / 'pinv' and every non-square system).

The truth of a least-squares / minimum-norm solve is numpy's float64 `pinv(a) @ b` on the inputs as rounded to
the dtype.  The forward error of a record is max |x - truth| / (|A^+|_2 max_k |b_k|_2), and its bound

    2 err_ref + 4 max(M, N) eps cond_2(A)

with err_ref the error of torch's CPU `pinv(a, rcond) @ b` in the same dtype on that record (the reference's own
composition, sugar.py:135) and cond_2 the ratio of the largest to the smallest singular value that counts.
Why |A^+| |b| and not |x|: a perturbation of A of size eps |A| moves the least-squares solution by up to
eps cond_2 (|x| + |A^+| |r|), r = b - A x (Wedin), and |x| and |A^+| |r| are both at most |A^+| |b|: against that
scale eps cond_2 is the error any backward-stable method may make, also when b is nearly orthogonal to the range
of A and x is small by cancellation (for square systems with a generic b the two scales agree within sqrt(M))."""
import functools
import numpy as np
import torch

NP = {'f32': np.float32, 'f64': np.float64}
TT = {'f32': torch.float32, 'f64': torch.float64}
CODE = {'f32': 0, 'f64': 1}
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
PLAIN, PINV = 0, 1
MAX_SWEEPS = 16
RECT_SHAPES = ((8, 3), (3, 8), (7, 5))
RECT_CONDS = {'f32': (1e1, 1e3), 'f64': (1e1, 1e6)}


def _orth(rng, n, m, k):
    """n matrices (m, k), k <= m, with orthonormal columns"""
    return np.linalg.qr(rng.standard_normal((n, m, m)))[0][:, :, :k]


def from_sigma(n, M, N, sigma, dn, seed):
    """U diag(sigma) V^T, M x N, sigma (n, min(M, N)) or (min(M, N),), built in float64 and rounded to the dtype"""
    rng = np.random.default_rng(seed)
    r = min(M, N)
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (n, r))
    u, v = _orth(rng, n, M, r), _orth(rng, n, N, r)
    return ((u * sigma[:, None, :]) @ v.transpose(0, 2, 1)).astype(NP[dn])


@functools.lru_cache(maxsize=None)
def rect_case(n, M, N, K, dn):
    """full-rank M x N records, singular values log-spaced from 1 to 1 / cond with the conds of RECT_CONDS taking
    turns, every record times its own power of two (2^-6 .. 2^6); and K right-hand sides.  Read-only."""
    r = min(M, N)
    conds = np.asarray(RECT_CONDS[dn])[np.arange(n) % len(RECT_CONDS[dn])]
    sigma = np.stack([np.logspace(0.0, -np.log10(c), r) if r > 1 else np.ones(1) for c in conds])
    a = from_sigma(n, M, N, sigma, dn, 1000 + 10 * M + N)
    a = np.ldexp(a, ((np.arange(n) % 13) - 6)[:, None, None]).astype(NP[dn])
    b = np.random.default_rng(2000 + 10 * M + N + K).standard_normal((n, M, K)).astype(NP[dn])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def truth(a, b, rcond=1e-15):
    """numpy float64 pinv(a, rcond) @ b per record (b None: the pseudo-inverse), cond_2 over the singular values
    that count, and the scale |A^+|_2 max_k |b_k|_2 of the forward error"""
    a64 = np.asarray(a, np.float64)
    s = np.linalg.svd(a64, compute_uv=False)
    keep = s > rcond * s.max(-1, keepdims=True)
    cond = s.max(-1) / np.where(keep, s, np.inf).min(-1)
    smin = np.where(keep, s, np.inf).min(-1)
    p = np.linalg.pinv(a64, rcond=rcond)
    if b is None:
        return p, cond, 1.0 / smin
    b64 = np.asarray(b, np.float64)
    return p @ b64, cond, np.sqrt((b64 * b64).sum(-2)).max(-1) / smin


def torch_ref(a, b, rcond=1e-15):
    """the reference's composition on the CPU in the dtype of a"""
    p = torch.linalg.pinv(torch.from_numpy(np.array(a)), rcond=rcond)
    return (p if b is None else p @ torch.from_numpy(np.array(b))).numpy()


def rec_err(x, tr, den):
    """max |x - truth| / den of every record; a non-finite result counts as inf"""
    x, tr = np.asarray(x, np.float64).reshape(len(x), -1), tr.reshape(len(tr), -1)
    with np.errstate(invalid='ignore'):
        e = np.abs(x - tr).max(-1) / den
    return np.where(np.isfinite(x).all(-1), e, np.inf)


def rect_excess(got, a, b, dn, rcond=1e-15, what=''):
    """err / (2 err_ref + 4 max(M, N) eps cond_2) of every record; prints the worst before anything is asserted"""
    M, N = a.shape[-2:]
    tr, cond, den = truth(a, b, rcond)
    err, eref = rec_err(got, tr, den), rec_err(torch_ref(a, b, rcond), tr, den)
    floor = 4.0 * max(M, N) * EPS[dn] * cond
    ex = err / (2.0 * eref + floor)
    i = int(np.argmax(ex))
    print(f'{what} {M}x{N} {dn}: worst err / bound = {ex[i]:.3g} (record {i}), worst err / (cond eps) = '
          f'{(err / (cond * EPS[dn])).max():.3g}, worst reference err / (cond eps) = {(eref / (cond * EPS[dn])).max():.3g}')
    return ex


def threshold_case(n, M, N, dn, rcond, seed):
    """records whose smallest singular value is rcond sigma_max 10^(+-1.5): even records keep it, odd ones drop
    it (never within a factor 4 of the threshold); the others log-spaced from 1 to 0.1"""
    r = min(M, N)
    sigma = np.tile(np.logspace(0.0, -1.0, r), (n, 1))
    sigma[:, -1] = rcond * 10.0 ** np.where(np.arange(n) % 2 == 0, 1.5, -1.5)
    a = from_sigma(n, M, N, sigma, dn, seed)
    s = np.linalg.svd(a.astype(np.float64), compute_uv=False)
    ratio = s[:, -1] / (rcond * s[:, 0])
    assert ((ratio > 4) | (ratio < 0.25)).all() and ((ratio > 1) == (np.arange(n) % 2 == 0)).all()
    b = np.random.default_rng(seed + 1).standard_normal((n, M, 3)).astype(NP[dn])
    return a, b


# ------------------------------------------------------------------------------------------------ the host entry
def _st(x):
    e = x.itemsize
    return (0, x.strides[0] // e, x.strides[1] // e, x.strides[2] // e)


def host_solve(L, a, b, flags, rcond=1e-15):
    """nfm_svd_solve_host on numpy records a (n, M, N), b (n, M, K) or None: (x (n, N, K), largest sweep count);
    more columns than one call takes go in blocks"""
    dn = 'f32' if a.dtype == np.float32 else 'f64'
    a = np.ascontiguousarray(a)
    n, M, N = a.shape
    K = M if b is None else b.shape[-1]
    out = np.empty((n, N, K), a.dtype)
    if b is None:
        rc = L.nfm_svd_solve_host(CODE[dn], M, N, K, flags, rcond, 1, n, a.ctypes.data, *_st(a), None, 0, 0, 0, 0,
                                  out.ctypes.data, *_st(out))
        assert rc >= 0, rc
        return out, rc
    b = np.ascontiguousarray(b)
    cap = L.nfm_svd_max_cols(CODE[dn], M, N)
    most = 0
    for c0 in range(0, K, cap):
        bv, ov = b[..., c0:c0 + cap], out[..., c0:c0 + cap]
        rc = L.nfm_svd_solve_host(CODE[dn], M, N, bv.shape[-1], flags, rcond, 1, n, a.ctypes.data, *_st(a),
                                  bv.ctypes.data, *_st(bv), ov.ctypes.data, *_st(ov))
        assert rc >= 0, rc
        most = max(most, rc)
    return out, most
