"""Helpers of the hard logm fixture (tests/golden/logm_hard.npz): the input classes, the validated high-precision
truth, the logarithm's condition number, and the bounds the tests hold the kernels and the torch route to.

Notation: K(A) is the D^2 x D^2 matrix of the Frechet derivative L_log(A),
cond_log(A) = ||K||_2 ||A||_F / ||log A||_F, m = max(1, cond_log).  Errors are Frobenius.

    logm, tier A        ||X - T||_F <= C_LOGM eps m ||T||_F
    logm, tier B        all NaN (Q22), or ||X - T||_F <= C_LOGM eps m^2 ||T||_F
    Frechet, tier A     ||L - L_true||_F <= C_LOGM D eps m^2 ||K||_2 ||E||_F
    logm_solve          ||X - T||_F <= C_LOGM D eps kappa_1(M) max(1, cond_log(M^-1 A)) ||T||_F

mpmath and scipy are needed by the generator only (and by the one test that validates a sample of the truths again);
they are imported where they are used.
"""
import os
import numpy as np

C_LOGM = 128                                    # tests/test_gpu_logm.py, profiles/logm_accuracy.md
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
ORDERS = {'f32': range(2, 9), 'f64': range(2, 8)}           # orders with a kernel and more than one entry
ROUTE_ORDERS = {'f32': (9, 12), 'f64': (8, 9, 12)}          # the torch route: tier-A classes only
FRECHET_ORDERS = range(2, 6)
PER_CLASS = 4
TIER_A, TIER_B = 0, 1
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'logm_hard.npz')

# class -> (tier, parameters per dtype); a record takes the parameter (index + D) % len
CLASSES = {
    'scale': (TIER_A, {'f32': (20, -20, 40, -40, 60, -60), 'f64': (20, -20, 40, -40, 60, -60)}),
    'graded': (TIER_A, {'f32': (3, 6), 'f64': (5, 10, 18)}),
    'rot': (TIER_A, {'f32': (0.3, 0.1), 'f64': (0.3, 0.1)}),
    'unip': (TIER_A, {'f32': (10, 100), 'f64': (10, 100)}),
    'tri': (TIER_A, {'f32': (10, 100), 'f64': (10, 100)}),
    'rotb': (TIER_B, {'f32': (0.03, 0.01, 0.003), 'f64': (1e-2, 1e-4, 1e-6)}),
    'nonnormal': (TIER_B, {'f32': (10, 100), 'f64': (10, 100)}),
}
SOLVE_M = {'f32': (3, 6), 'f64': (5, 10)}       # the graded M of logm_solve: kappa_1(M) to 1e4 / 1e8


def make(cls, D, par, rng):
    """one float64 matrix of the class (rounded to the record's dtype by the caller)"""
    from scipy.linalg import expm
    r = rng.standard_normal
    if cls == 'scale':
        return expm(0.5 * r((D, D))) * 2.0 ** par
    if cls == 'graded':
        V = np.eye(D) + 0.3 * r((D, D))
        return V @ np.diag(2.0 ** np.linspace(-par, par, D)) @ np.linalg.inv(V)
    if cls in ('rot', 'rotb'):
        g = r((D, D))
        s = g - g.T
        return expm(s * ((np.pi - par) / np.abs(np.linalg.eigvals(s).imag).max()))
    if cls == 'unip':
        return np.eye(D) + par * np.triu(r((D, D)), 1) / D
    if cls == 'tri':
        return np.diag(rng.uniform(0.5, 2, D)) + par * np.triu(r((D, D)), 1) / D
    if cls == 'nonnormal':
        Q = np.linalg.qr(r((D, D)))[0]
        return Q @ (np.diag(rng.uniform(0.5, 2, D)) + par * np.triu(r((D, D)), 1) / D) @ Q.T
    raise ValueError(cls)


# ---------------------------------------------------------------------------------------------------------------
# the truth: mpmath, validated (mpmath.logm is a Denman-Beavers iteration itself: it returns wrong logarithms
# within 0.1 rad of pi without an error, and does not converge on graded matrices)

def _mp_max(M):
    return max(abs(M[i, j]) for i in range(M.rows) for j in range(M.cols))


def mp_validate(L, A):
    """(residual ||expm(L) - A||_max / ||A||_max, largest imaginary part of L), as floats"""
    import mpmath
    res = _mp_max(mpmath.expm(L) - A) / _mp_max(A)
    im = max(abs(mpmath.im(L[i, j])) for i in range(L.rows) for j in range(L.cols))
    return float(res), float(im)


def mp_logm(A, tol=1e-30):
    """validated principal logarithm of an mpmath matrix at the working precision: `mpmath.logm`, then the
    eigendecomposition V log(Lambda) V^-1; the first whose residual and imaginary part are <= tol.
    Returns (real mpmath matrix, residual, route) or (None, None, 'none')."""
    import mpmath

    def by_logm():
        return mpmath.logm(A)

    def by_eig():
        E, ER = mpmath.eig(A)
        return ER * mpmath.diag([mpmath.log(e) for e in E]) * mpmath.inverse(ER)

    for name, f in (('logm', by_logm), ('eig', by_eig)):
        try:
            L = f()
            res, im = mp_validate(L, A)
        except Exception:       # NoConvergence, ZeroDivisionError of a defective eigenbasis, ...
            continue
        if res <= tol and im <= tol:
            return L.apply(mpmath.re), max(res, im), name
    return None, None, 'none'


def mp_of(a):
    import mpmath
    return mpmath.matrix(np.asarray(a, dtype=np.float64).tolist())


def mp_to_np(L):
    return np.array([[float(L[i, j]) for j in range(L.cols)] for i in range(L.rows)])


def mp_frechet(A, E, h_rel=1e-20):
    """L_log(A, E) by the central difference of validated logarithms, h = h_rel ||A||_max (relative, so that the
    step is as small against a matrix of size 2^-60 as against one of size 1); run at 80 digits"""
    import mpmath
    h = mpmath.mpf(h_rel) * _mp_max(A)
    Lp, _, _ = mp_logm(A + h * E)
    Lm, _, _ = mp_logm(A - h * E)
    if Lp is None or Lm is None:
        return None
    return (Lp - Lm) / (2 * h)


def klog_norm(T):
    """||K(A)||_2 from T = log A in float64: K(A) is the inverse of the matrix of L_exp(T), whose columns are
    scipy's `expm_frechet` (scaling and squaring; sound on defective T, which the block-matrix trick is not)"""
    from scipy.linalg import expm_frechet
    D = T.shape[0]
    Kexp = np.empty((D * D, D * D))
    for q in range(D * D):
        E = np.zeros(D * D)
        E[q] = 1
        Kexp[:, q] = expm_frechet(T, E.reshape(D, D), compute_expm=False).ravel()
    return 1.0 / np.linalg.svd(Kexp, compute_uv=False)[-1], Kexp


# ---------------------------------------------------------------------------------------------------------------
# the fixture and the bounds

def fro(x):
    return np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum((-2, -1)))


def load():
    return np.load(PATH)


def records(g, dt, D):
    """the arrays of one (dtype, order): x, true, nK, cl, cls, par, tier, res (and E, L at the Frechet orders)"""
    keys = ['x', 'true', 'nK', 'cl', 'cls', 'par', 'tier', 'res'] + (['E', 'L'] if D in FRECHET_ORDERS else [])
    return {k: g[f'{k}_{dt}_{D}'] for k in keys}


def m_of(cl):
    return np.maximum(1.0, cl)


def logm_ratio(k, rec, dt):
    """per record: ||k - T||_F / ||T||_F in units of eps m (tier A is held to <= C_LOGM); NaN for a NaN result"""
    k = np.asarray(k, dtype=np.float64)
    return fro(k - rec['true']) / fro(rec['true']) / (EPS[dt] * m_of(rec['cl']))


def frechet_ratio(l, rec, dt):
    """per record: ||l - L_true||_F in units of D eps m^2 ||K||_2 ||E||_F (tier A is held to <= C_LOGM)"""
    l = np.asarray(l, dtype=np.float64)
    D = l.shape[-1]
    return fro(l - rec['L']) / (D * EPS[dt] * m_of(rec['cl']) ** 2 * rec['nK'] * fro(rec['E']))


def check_logm(k, rec, dt, c=C_LOGM):
    """-> (ok per record, ratio per record, outcome per record: 'A', 'B:nan', 'B:m2' or 'FAIL')"""
    k = np.asarray(k, dtype=np.float64)
    r = logm_ratio(k, rec, dt)
    nan = np.isnan(k).all((-2, -1))
    anynan = np.isnan(k).any((-2, -1))
    m = m_of(rec['cl'])
    ok, what = [], []
    for i in range(len(r)):
        if rec['tier'][i] == TIER_A:
            good = (not anynan[i]) and r[i] <= c
            what.append('A' if good else 'FAIL')
        elif nan[i]:
            good = True
            what.append('B:nan')
        else:
            good = (not anynan[i]) and r[i] <= c * m[i]
            what.append('B:m2' if good else 'FAIL')
        ok.append(good)
    return np.array(ok), r, what


def worst_by_class(r, rec):
    """{'class/tier': worst finite ratio}  (the stored class of 'rotb' is 'rot': tier B)"""
    out = {}
    for c, t in dict.fromkeys(zip(rec['cls'].tolist(), rec['tier'].tolist())):
        v = r[(rec['cls'] == c) & (rec['tier'] == t) & np.isfinite(r)]
        out[f'{c}/{"AB"[t]}'] = float(v.max()) if len(v) else float('nan')
    return out
