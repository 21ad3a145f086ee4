"""Reference model of `sym.sym_funm` (spectral functions of compact symmetric matrices) and of its gradient, numpy
only, written from the definitions: Y = V f(max(L, min)) V^T and the Daleckii-Krein gradient
S = V [(V^T G V) o F] V^T, F_kl = (f o max(., min))[l_k, l_l].

High precision: float32 results are judged against numpy's float64 `eigh` of the float32 input, float64 results
against a cyclic Jacobi eigensolver in numpy.longdouble (64-bit mantissa, asserted by `high_ok`).

Per record the model returns Y, S and the conditioning numbers of the bounds:
    L  = max_kl |F_kl|
    M2 = sup |f''| / 2 over the clamped spectrum's interval (attained at an endpoint for these functions), plus
         L_f / gap when the clamp is active (some eigenvalue below `min`), gap = min_i |l_i - min|
    forward   ||Y^ - Y||_F <= C n eps (L ||A||_2 + ||Y||_2)
    gradient  ||S^ - S||_F <= C n eps (M2 ||A||_2 + L) ||G||_F
(for exp, n + max|l| in place of n), C = 16: the constant of tests/_eig_ref.py, the bar of eig_sym's fast arithmetic.
The divided differences of the model are NOT the kernels' closed forms: the plain quotient where the pair is well
separated, the midpoint Taylor series f[a, b] = sum_j f^(2j+1)(m) h^(2j) / (2j+1)!  (m the midpoint, h the half
difference) where it is not.
"""
import functools
import math
import numpy as np

NP = {'f32': np.float32, 'f64': np.float64}
HP = {'f32': np.float64, 'f64': np.longdouble}
C = 16.0
FUNCS = ('exp', 'log', 'sqrt', 'rsqrt', 'pow', 'clamp')
FAMILIES = ('normal', 'graded', 'repeated', 'cluster', 'isotropic', 'rank1', 'scaled')
SCALED_FUNCS = ('sqrt', 'rsqrt', 'log', 'clamp')          # the functions the `scaled` family is for
POW_P = 1.7
CLAMP_MIN = 0.75
NB = 3 * 256 + 5          # several tiles of the largest tile size and a ragged tail


def eps_of(dn):
    return float(np.finfo(NP[dn]).eps)


def high_ok():
    return np.finfo(np.longdouble).eps <= 2.0 ** -63


# ------------------------------------------------------------------------------------------------ compact storage
def index(n):
    r = list(range(n)) + [i for i in range(n) for j in range(i + 1, n)]
    c = list(range(n)) + [j for i in range(n) for j in range(i + 1, n)]
    return np.asarray(r), np.asarray(c)


def pack(full, off=1.0):
    n = full.shape[-1]
    r, c = index(n)
    out = full[..., r, c].copy()
    out[..., n:] *= off
    return out


def unpack(comp, n, off=1.0):
    r, c = index(n)
    v = np.array(comp, copy=True)
    v[..., n:] *= off
    full = np.zeros(comp.shape[:-1] + (n, n), comp.dtype)
    full[..., r, c] = v
    full[..., c, r] = v
    return full


# ------------------------------------------------------------------------------------------------ input families
def _orth(rng, nb, n):
    q, r = np.linalg.qr(rng.standard_normal((nb, n, n)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def _from_spectrum(rng, lam):
    q = _orth(rng, *lam.shape)
    a = np.einsum('bij,bj,bkj->bik', q, lam, q)
    return (a + a.swapaxes(-1, -2)) / 2


def family(name, dn, rng, nb, n):
    """nb float64 SPD records of one family (rounded to the dtype by the caller)"""
    if name == 'normal':                               # cond <= 10
        return _from_spectrum(rng, rng.uniform(0.5, 5.0, (nb, n)))
    if name == 'graded':                               # cond 1e4 / 1e10, log-spaced from 2 down
        dec = 4.0 if dn == 'f32' else 10.0
        lam = 2.0 * 10.0 ** (-dec * np.arange(n) / max(n - 1, 1)) * np.ones((nb, 1))
        return _from_spectrum(rng, lam)
    if name == 'repeated':                             # two groups, exactly repeated
        lam = np.where(np.arange(n) < n // 2, 0.5, 2.0) * np.ones((nb, 1))
        return _from_spectrum(rng, lam)
    if name == 'cluster':                              # 1 +- 1e-5 / 1e-11
        d = 1e-5 if dn == 'f32' else 1e-11
        return _from_spectrum(rng, 1.0 + d * rng.uniform(-1.0, 1.0, (nb, n)))
    if name == 'isotropic':                            # c I exactly
        return np.eye(n) * rng.uniform(0.5, 4.0, (nb, 1, 1))
    if name == 'rank1':                                # v v^T + shift, |v|^2 <= 8
        v = rng.standard_normal((nb, n))
        v *= np.minimum(1.0, np.sqrt(8.0) / np.linalg.norm(v, axis=1))[:, None]
        return v[:, :, None] * v[:, None, :] + np.eye(n) * rng.uniform(0.25, 1.5, (nb, 1, 1))
    if name == 'scaled':                               # normal times 2^+-40 / 2^+-300
        e = 40 if dn == 'f32' else 300
        return family('normal', dn, rng, nb, n) * (2.0 ** (e * rng.choice([-1.0, 1.0], (nb, 1, 1))))
    raise ValueError(name)


def families_of(fn):
    return tuple(f for f in FAMILIES if f != 'scaled' or fn in SCALED_FUNCS)


def fn_args(fn):
    """(p, min) of the plain call of each function"""
    return (POW_P if fn == 'pow' else None), (CLAMP_MIN if fn == 'clamp' else None)


@functools.lru_cache(maxsize=None)
def batch(dn, n, fn, nb=NB):
    """(compact records of the dtype, {family: slice}): every family of `fn` in one batch.  exp gets the records
    shifted by -2 I (eigenvalues of both signs, all <= 40); the scaled clamp records are clamped at their own scale
    by the caller's single `min`, so they sit wholly above or wholly below it."""
    fams = families_of(fn)
    seed = 1000 * n + 10 * FUNCS.index(fn) + (dn == 'f64')
    rng = np.random.default_rng(seed)
    per = nb // len(fams)
    parts, cells, at = [], {}, 0
    for k, f in enumerate(fams):
        m = per if k + 1 < len(fams) else nb - at
        a = family(f, dn, rng, m, n)
        if fn == 'exp':
            a = a - 2.0 * np.eye(n)
        parts.append(a)
        cells[f] = slice(at, at + m)
        at += m
    comp = pack(np.concatenate(parts)).astype(NP[dn])
    comp.setflags(write=False)
    return comp, cells


def cotangent(dn, n, nb=NB, seed=7):
    """a random symmetric cotangent in compact storage"""
    rng = np.random.default_rng(seed + n)
    g = rng.standard_normal((nb, n * (n + 1) // 2)).astype(NP[dn])
    g.setflags(write=False)
    return g


# ------------------------------------------------------------------------------------------------ eigensolvers
def jacobi_eigh(a, sweeps=40):
    """cyclic Jacobi in the precision of `a` (batched, n <= 16): (eigenvalues ascending, eigenvectors in columns)"""
    a = np.array(a, copy=True)
    nb, n, _ = a.shape
    assert n <= 16
    T = a.dtype.type
    v = np.broadcast_to(np.eye(n, dtype=a.dtype), a.shape).copy()
    eps = np.finfo(a.dtype).eps
    scale = np.sqrt((a * a).sum((1, 2)))
    for _ in range(sweeps):
        off = np.sqrt(((a * (1 - np.eye(n, dtype=a.dtype))) ** 2).sum((1, 2)))
        if np.all(off <= eps * scale / 4):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[:, p, q]
                nz = np.abs(apq) > 0
                den = np.where(nz, 2 * apq, T(1))
                with np.errstate(over='ignore'):            # a huge theta is a rotation by zero
                    theta = (a[:, q, q] - a[:, p, p]) / den
                    t = np.where(theta >= 0, T(1), T(-1)) / (np.abs(theta) + np.hypot(theta, T(1)))
                t = np.where(nz, t, T(0))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                ap, aq = a[:, :, p].copy(), a[:, :, q].copy()
                a[:, :, p] = c[:, None] * ap - s[:, None] * aq
                a[:, :, q] = s[:, None] * ap + c[:, None] * aq
                ap, aq = a[:, p, :].copy(), a[:, q, :].copy()
                a[:, p, :] = c[:, None] * ap - s[:, None] * aq
                a[:, q, :] = s[:, None] * ap + c[:, None] * aq
                vp, vq = v[:, :, p].copy(), v[:, :, q].copy()
                v[:, :, p] = c[:, None] * vp - s[:, None] * vq
                v[:, :, q] = s[:, None] * vp + c[:, None] * vq
    lam = np.diagonal(a, axis1=1, axis2=2).copy()
    order = np.argsort(lam, axis=1)
    lam = np.take_along_axis(lam, order, 1)
    v = np.take_along_axis(v, order[:, None, :], 2)
    return lam, v


def eigh_hp(dn, full):
    """eigendecomposition of the dtype's records in the high precision of the dtype"""
    if dn == 'f32':
        return np.linalg.eigh(full.astype(np.float64))
    return jacobi_eigh(full.astype(np.longdouble))


# ------------------------------------------------------------------------------------------------ scalar pieces
def _deriv(fn, p, k, x):
    """k-th derivative of f at x (k >= 0), in the precision of x"""
    if fn == 'exp':
        return np.exp(x)
    if fn == 'clamp':
        return x if k == 0 else (np.ones_like(x) if k == 1 else np.zeros_like(x))
    if fn == 'log':
        if k == 0:
            return np.log(x)
        return (-1.0) ** (k - 1) * math.factorial(k - 1) / x ** k
    q = {'sqrt': 0.5, 'rsqrt': -0.5, 'pow': p}[fn]
    coef = x.dtype.type(1)
    for j in range(k):
        coef = coef * x.dtype.type(q - j)
    if fn == 'sqrt' and k == 0:
        return np.sqrt(x)
    return coef * np.power(x, x.dtype.type(q) - k)


def divdiff_hp(fn, p, a, b):
    """f[a, b] in the precision of a, b (no clamp): quotient for separated pairs, midpoint Taylor series otherwise"""
    m, h = (a + b) / 2, (a - b) / 2
    size = np.ones_like(a) if fn == 'exp' else np.maximum(np.abs(a), np.abs(b))
    near = np.abs(h) <= 1e-2 * size
    ms = np.where(near, m, np.ones_like(m))
    series = np.zeros_like(a)
    hs = np.where(near, h, np.zeros_like(h))
    for j in range(8):                               # the first term left out is (1e-2)^16 / 17!: below any eps here
        series = series + _deriv(fn, p, 2 * j + 1, ms) * hs ** (2 * j) / math.factorial(2 * j + 1)
    with np.errstate(all='ignore'):
        quot = (_deriv(fn, p, 0, a) - _deriv(fn, p, 0, b)) / np.where(a == b, np.ones_like(a), a - b)
    return np.where(near, series, quot)


def model(dn, fn, comp, p=None, vmin=None, g=None):
    """the high-precision model for compact records `comp` of dtype dn (and a compact cotangent g).
    dict: Y, S (full symmetric, high precision; S None without g), L, M2, normA, normY, lam_max, bad (records
    outside the domain: their Y / S are NaN)."""
    hp = HP[dn]
    vmin = None if vmin is None else float(NP[dn](vmin))          # the clamp is a number of the dtype, as in torch.clamp
    n = int((math.isqrt(1 + 8 * comp.shape[-1]) - 1) // 2)
    full = unpack(np.asarray(comp), n)
    lam, v = eigh_hp(dn, full)
    lam, v = lam.astype(hp), v.astype(hp)
    lc = lam if vmin is None else np.maximum(lam, hp(vmin))
    if fn in ('log', 'rsqrt') or (fn == 'pow' and p < 0):
        bad = ~(lc > 0).all(1)
    elif fn in ('sqrt', 'pow'):
        bad = ~(lc >= 0).all(1)
    else:
        bad = np.zeros(len(lc), bool)
    bad |= ~np.isfinite(np.asarray(comp, np.float64)).all(1)
    ls = np.where(bad[:, None], np.ones_like(lc), lc)
    f = _deriv(fn, p, 0, ls)
    Y = np.einsum('bik,bk,bjk->bij', v, f, v)
    a2, b2 = np.broadcast_arrays(lam[:, :, None], lam[:, None, :])
    ca, cb = np.broadcast_arrays(ls[:, :, None], ls[:, None, :])
    F0 = divdiff_hp(fn, p, ca, cb)
    F = F0
    if vmin is not None:
        eq = a2 == b2
        fac = np.where(eq, (a2 >= hp(vmin)).astype(hp), (ca - cb) / np.where(eq, np.ones_like(a2), a2 - b2))
        F = F0 * fac
    L = np.abs(F).max((1, 2)).astype(np.float64)
    lo, hi = ls.min(1), ls.max(1)
    with np.errstate(all='ignore'):
        M2 = np.maximum(np.abs(_deriv(fn, p, 2, lo)), np.abs(_deriv(fn, p, 2, hi))).astype(np.float64) / 2
        if vmin is not None:
            active = (lam < hp(vmin)).any(1)
            gap = np.abs(lam - hp(vmin)).min(1).astype(np.float64)
            Lf = np.maximum(np.abs(_deriv(fn, p, 1, lo)), np.abs(_deriv(fn, p, 1, hi))).astype(np.float64)
            M2 = M2 + np.where(active, Lf / np.where(gap > 0, gap, 1.0), 0.0)
    S = None
    if g is not None:
        G = unpack(np.asarray(g).astype(hp), n, off=0.5)
        W = np.einsum('bik,bij,bjl->bkl', v, G, v) * F
        S = np.einsum('bik,bkl,bjl->bij', v, W, v)
        S[bad] = np.nan
    Y[bad] = np.nan
    return dict(Y=Y, S=S, L=L, M2=M2, normA=np.abs(lam).max(1).astype(np.float64),
                normY=np.abs(f).max(1).astype(np.float64), lam_max=np.abs(ls).max(1).astype(np.float64), bad=bad, n=n)


def _fro(x):
    return np.sqrt((np.asarray(x, np.float64) ** 2).sum((-1, -2)))


def forward_ratio(dn, fn, mod, got):
    """per record: ||Y^ - Y||_F over n eps (L ||A||_2 + ||Y||_2) (n + max|l| for exp); the bar is C"""
    n = mod['n']
    hp = HP[dn]
    err = _fro(unpack(np.asarray(got).astype(hp), n) - mod['Y'])
    fac = n + (mod['lam_max'] if fn == 'exp' else 0.0)
    return err / (fac * eps_of(dn) * (mod['L'] * mod['normA'] + mod['normY']))


def backward_ratio(dn, fn, mod, g, got):
    """per record: ||S^ - S||_F over n eps (M2 ||A||_2 + L) ||G||_F; the bar is C"""
    n = mod['n']
    hp = HP[dn]
    err = _fro(unpack(np.asarray(got).astype(hp), n, off=0.5) - mod['S'])
    G = _fro(unpack(np.asarray(g).astype(np.float64), n, off=0.5))
    fac = n + (mod['lam_max'] if fn == 'exp' else 0.0)
    return err / (fac * eps_of(dn) * (mod['M2'] * mod['normA'] + mod['L']) * G)


@functools.lru_cache(maxsize=None)
def truth(dn, n, fn):
    """model of batch(dn, n, fn) with the plain arguments of fn and the shared cotangent; computed once"""
    comp, _ = batch(dn, n, fn)
    p, vmin = fn_args(fn)
    return model(dn, fn, comp, p, vmin, cotangent(dn, n))
