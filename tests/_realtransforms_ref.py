"""Dense float64 matrices of the real transforms, written from their definitions, and the error bound the
realtransforms tests hold results to.

    matrix('dct' | 'dst', type, norm, N)[k, n]:  y = M x

"backward" (unnormalised) matrices:
    DCT-II   2 cos(pi k (2n+1) / 2N)
    DCT-III  x0 + 2 sum_{n>=1} x_n cos(pi (2k+1) n / 2N)
    DCT-I    x0 + (-1)^k x_{N-1} + 2 sum_{n=1..N-2} x_n cos(pi k n / (N-1))
    DST-II   2 sin(pi (k+1) (2n+1) / 2N)
    DST-III  (-1)^k x_{N-1} + 2 sum_{n<N-1} x_n sin(pi (2k+1) (n+1) / 2N)
    DST-I    2 sin(pi (k+1) (n+1) / (N+1))
'forward' divides by 2L (L = N; N - 1 for DCT-I; N + 1 for DST-I).  'ortho' divides by sqrt(2L) and rescales
the end terms so that M is orthogonal: the first output (DCT-II) / last output (DST-II) by 1 / sqrt(2), the
first input (DCT-III) / last input (DST-III) by sqrt(2), both ends of DCT-I on both sides.  'ortho_scipy' is the
reference's own convention: 'ortho' for every DCT and for type I; for DST-II / DST-III the correction sits on
the FIRST output / input instead of the last.  The scalings are pinned by tests/golden/realtransforms.npz.
"""
import numpy as np

KINDS = ('dct', 'dst')
TYPES = (1, 2, 3)
NORMS = ('backward', 'forward', 'ortho', 'ortho_scipy')
FLIPNORM = {'backward': 'forward', 'forward': 'backward', 'ortho': 'ortho', 'ortho_scipy': 'ortho_scipy'}
FLIPTYPE = {1: 1, 2: 3, 3: 2}


def cospi_frac(a, b):
    """cos(pi a / b) for integer arrays a and an integer b > 0, with the angle folded in integers into
    [0, pi/4]: every entry then has a RELATIVE error of an ulp or two and the zeros of the cosine are exact
    zeros (np.cos(np.pi * x) is only absolutely accurate: 6e-17 where the matrix has a zero, which the
    per-element bound below cannot tell from a wrong result)."""
    a = np.asarray(a, dtype=np.int64) % (2 * b)
    a = np.where(a > b, 2 * b - a, a)
    neg = 2 * a > b
    a = np.where(neg, b - a, a)
    v = np.where(4 * a <= b, np.cos(np.pi * a / b), np.sin(np.pi * (b - 2 * a) / (2 * b)))
    return np.where(neg, -v, v)


def sinpi_frac(a, b):
    """sin(pi a / b) = cos(pi (b - 2a) / 2b)"""
    return cospi_frac(b - 2 * np.asarray(a, dtype=np.int64), 2 * b)


def backward_matrix(kind, type, N):
    k = np.arange(N, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    if kind == 'dct':
        if type == 2:
            return 2 * cospi_frac(k * (2 * n + 1), 2 * N)
        if type == 3:
            M = 2 * cospi_frac((2 * k + 1) * n, 2 * N)
            M[:, 0] = 1
            return M
        if N < 2:
            raise ValueError('DCT-I needs at least two points')
        M = 2 * cospi_frac(k * n, N - 1)
        M[:, 0] = 1
        M[:, -1] = sign
        return M
    if type == 2:
        return 2 * sinpi_frac((k + 1) * (2 * n + 1), 2 * N)
    if type == 3:
        M = 2 * sinpi_frac((2 * k + 1) * (n + 1), 2 * N)
        M[:, -1] = sign
        return M
    return 2 * sinpi_frac((k + 1) * (n + 1), N + 1)


def matrix(kind, type, norm, N):
    M = backward_matrix(kind, type, N)
    norm = norm or 'backward'
    if type == 1 and norm == 'ortho_scipy':
        norm = 'ortho'
    L = N if type != 1 else (N - 1 if kind == 'dct' else N + 1)
    if norm == 'backward':
        return M
    if norm == 'forward':
        return M / (2 * L)
    M = M / np.sqrt(2 * L)
    end = 0 if (kind == 'dct' or norm == 'ortho_scipy') else -1
    if type == 2:
        M[end, :] /= np.sqrt(2)
    elif type == 3:
        M[:, end] *= np.sqrt(2)
    elif kind == 'dct':
        M[:, 0] *= np.sqrt(2)
        M[:, -1] *= np.sqrt(2)
        M[0, :] /= np.sqrt(2)
        M[-1, :] /= np.sqrt(2)
    return M


def inverse_matrix(kind, type, norm, N):
    """what idct / idst apply: the flipped type under the flipped norm"""
    return matrix(kind, FLIPTYPE[type], FLIPNORM[norm or 'backward'], N)


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def bound(M, x, dtype, axis=-1, factor=1.0):
    """Per output element (N + 6) eps sum_n |M_kn| |x_n| + the smallest normal number: the recursive-summation
    bound of an N-term sum (N eps) with six ulps for the rounding of the coefficient (cospi / sinpi, its
    argument), of the end-term factors and of the output factor.  x: lines along `axis`."""
    N = M.shape[0]
    ax = np.moveaxis(np.abs(np.asarray(x, dtype=np.float64)), axis, -1)
    b = (N + 6) * eps_of(dtype) * (ax @ np.abs(M).T) * factor + float(np.finfo(dtype).tiny)
    return np.moveaxis(b, -1, axis)


def apply(M, x, axis=-1):
    """M applied to the lines of x along `axis`, in float64"""
    xx = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    return np.moveaxis(xx @ M.T, -1, axis)


def ratio(got, want, b):
    """worst |got - want| / bound (NaN-safe: a NaN where none is expected is inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    err = np.where(np.isnan(err), np.inf, err)
    return float(np.max(err / b)) if err.size else 0.0
