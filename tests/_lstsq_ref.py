"""Inputs, truths and the bound shared by tests/test_lstsq_host.py and tests/test_gpu_lstsq.py (the tall
least-squares solves of `sugar`: `nfm_lstsq_solve`, more than 8 rows, at most 8 columns).

Truth, error and scale are those of tests/_svd_ref.py: numpy's float64 `pinv(a, rcond) @ b` on the inputs as
rounded to the dtype, err = max |x - truth| / (|A^+|_2 max_k |b_k|_2) per record, err_ref the same for torch's CPU
`pinv(a, rcond) @ b` in the dtype.  The bound of a record is

    2 err_ref + 4 N eps cond_2(A)

with N, the number of COLUMNS, in the floor -- not _svd_ref's max(M, N): the streamed QR makes N rotations per row
and its backward error does not grow with M the way a floor of 4 M eps would allow (at M = 257 that floor would
pass with three orders of magnitude to spare and hold nothing).  A numpy emulation of the streaming rotations in
the working dtype, finished by torch's `pinv` of R, stays at or below 0.32 of this bound on the shapes of the
tests, worst at N <= 2."""
import functools
import numpy as np
import _svd_ref as V

NP, TT, CODE, EPS = V.NP, V.TT, V.CODE, V.EPS
MAX_SWEEPS = V.MAX_SWEEPS
MAX_ROWS = 4096
# (M, N, K); K None = the column cap of the dtype at that N
SHAPES = ((9, 1, 1), (9, 8, 2), (17, 3, 1), (33, 6, 3), (64, 7, 1), (257, 3, 2), (200, 8, None))


@functools.lru_cache(maxsize=None)
def tall_case(n, M, N, K, dn, seed, exps=None):
    """full-rank M x N records, singular values log-spaced from 1 to 1 / cond with the conds of V.RECT_CONDS
    taking turns, every record times its own power of two (2^-6 .. 2^6, or the tuple `exps`); b standard normal.
    Read-only."""
    conds = np.asarray(V.RECT_CONDS[dn])[np.arange(n) % len(V.RECT_CONDS[dn])]
    sigma = np.stack([np.logspace(0.0, -np.log10(c), N) if N > 1 else np.ones(1) for c in conds])
    a = V.from_sigma(n, M, N, sigma, dn, seed)
    k = (np.arange(n) % 13) - 6 if exps is None else np.asarray(exps)
    a = np.ldexp(a, k[:, None, None]).astype(NP[dn])
    b = np.random.default_rng(seed + 1).standard_normal((n, M, K)).astype(NP[dn])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def rank5_case(n, dn, seed):
    """33 x 6 records of rank exactly 5: products of small integer matrices, exact in both dtypes"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(-3, 4, (n, 33, 5)) @ rng.integers(-3, 4, (n, 5, 6))).astype(np.float64)
    assert (np.linalg.matrix_rank(a) == 5).all() and np.abs(a).max() < 2 ** 20
    b = rng.standard_normal((n, 33, 2)).astype(NP[dn])
    return a.astype(NP[dn]), b


def excess(got, a, b, dn, rcond=1e-15, what='', ref=None):
    """err / (2 err_ref + 4 N eps cond_2) of every record; prints the worst before anything is asserted.
    `ref`: the reference-side result when it is not torch's CPU composition (a golden array)."""
    M, N = a.shape[-2:]
    tr, cond, den = V.truth(a, b, rcond)
    ref = V.torch_ref(a, b, rcond) if ref is None else ref
    err, eref = V.rec_err(got, tr, den), V.rec_err(ref, tr, den)
    ex = err / (2.0 * eref + 4.0 * N * EPS[dn] * cond)
    i = int(np.argmax(ex))
    print(f'{what} {M}x{N} K={b.shape[-1]} {dn}: worst err / bound = {ex[i]:.3g} (record {i}), worst err / (cond eps) = '
          f'{(err / (cond * EPS[dn])).max():.3g}, worst reference err / (cond eps) = {(eref / (cond * EPS[dn])).max():.3g}')
    return ex


# ------------------------------------------------------------------------------------------------ the host entry
def _st(x):
    e = x.itemsize
    return (0, x.strides[0] // e, x.strides[1] // e, x.strides[2] // e)


def host_solve(L, a, b, rcond=1e-15):
    """nfm_lstsq_solve_host on numpy records a (n, M, N), b (n, M, K): (x (n, N, K), largest sweep count); more
    columns than one call takes go in blocks"""
    dn = 'f32' if a.dtype == np.float32 else 'f64'
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    n, M, N = a.shape
    K = b.shape[-1]
    out = np.empty((n, N, K), a.dtype)
    cap = L.nfm_lstsq_max_cols(CODE[dn], N)
    most = 0
    for c0 in range(0, K, cap):
        bv, ov = b[..., c0:c0 + cap], out[..., c0:c0 + cap]
        rc = L.nfm_lstsq_solve_host(CODE[dn], M, N, bv.shape[-1], rcond, 1, n, a.ctypes.data, *_st(a),
                                    bv.ctypes.data, *_st(bv), ov.ctypes.data, *_st(ov))
        assert rc >= 0, rc
        most = max(most, rc)
    return out, most
