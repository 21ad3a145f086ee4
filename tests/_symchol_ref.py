"""Reference model of the Cholesky functions of `sym` (sym_chol, sym_chol_apply, sym_logdet, sym_mahalanobis,
sym_gauss_logpdf and the gradients of the three scalars): inputs, a high-precision model and per-record first-order
error bounds.  numpy only, written from the definitions.

High precision: float32 results are judged in float64, float64 results in numpy.longdouble (64-bit mantissa, asserted
by `_symfun_ref.high_ok`); the factorisation, the triangular inverse and every product below are plain loops over the
order, vectorised over the batch, in the precision of their argument -- so the same routines in the WORKING precision
are the "plain numpy Cholesky" the bounds are validated with (`plain`).

The bounds (per record, elementwise; gamma = (n + 2) eps, P = |L||L^T|, y = L^-1 v, w = A^-1 v, q = y^T y, d = sqrt q):
    factor      |A - L^ L^^T|                 <= gamma P                                  (Higham, Theorem 10.3)
    logdet      |err|                         <= gamma sum_ij |A^-1|_ij P_ij + 2 gamma sum_i |log L_ii|
    the factor's own error, to first order    |dL| <= gamma |L| (|L^-1| P |L^-T|)
    'Linv'      |err| <= |L^-1| |dL| |y| + gamma |L^-1| |L| |y|         ('LTinv': the same with every factor transposed)
    'L'         |err| <= gamma |L| |v| + |dL| |v|                       ('LT': transposed)
    squared Mahalanobis  |err| <= gamma (|w|^T P |w| + 2 |w|^T |L| |y| + q);  the root: that over 2 d
    logpdf      half the sum of the logdet and the squared-Mahalanobis bounds
    gradients   |dA^-1| <= 3 gamma |A^-1| P |A^-1|, |dw| <= 3 gamma |A^-1| P |w|, carried through
                S = g A^-1 | -g w w^T | -(g / 2d) w w^T | -g (A^-1 - w w^T) / 2 and g_v = 2 g w | (g / d) w | -g w
                by the product rule (the root's coefficient g / 2d carries the error of d) and scaled by |g|.
(|dL|: dL = L tril(L^-1 dA L^-T) with |dA| <= gamma P, so the product is ordered |L| first; the transposed ops use its
transpose.)  The bar is a ratio <= 1 in every cell: these are rigorous first-order bounds, not measurements.  They hold
while kappa_2(D^-1 A D^-1) n eps <= 1/16, D = sqrt diag A (`judged`), which every record of `batch` satisfies.
"""
import functools
import numpy as np
import _symfun_ref as R

NP, HP = R.NP, R.HP
NB = 1200                                  # not a multiple of 64, more than two tiles
ORDERS = (1, 2, 3, 4, 6, 8)
CELLS = ('wishart', 'spectra', 'graded', 'isotropic', 'equicorrelated', 'scaled')
APPLY = ('L', 'LT', 'Linv', 'LTinv')
SCALARS = ('logdet', 'maha', 'maha_sqrt', 'logpdf')
# include/nfm_hip.h: NFM_CHOL_*
CODE = {'factor': 0, 'L': 1, 'LT': 2, 'Linv': 3, 'LTinv': 4, 'logdet': 5, 'maha': 6, 'maha_sqrt': 7, 'logpdf': 8}
FACTORED = 16
LOG_2PI = np.longdouble('1.8378770664093454835606594728112353')


def gamma(dn, n):
    return (n + 2) * R.eps_of(dn)


# ------------------------------------------------------------------------------------------------ inputs
def _wishart(rng, nb, n, delta=0.25):
    g = rng.standard_normal((nb, n, n))
    return g @ g.swapaxes(-1, -2) / n + delta * np.eye(n)


def cell(name, dn, rng, nb, n):
    """nb float64 SPD records of one cell (rounded to the dtype by the caller)"""
    if name == 'wishart':
        return _wishart(rng, nb, n)
    if name == 'spectra':                              # Q diag(logspace(0, -p)) Q^T
        p = 3.0 if dn == 'f32' else 10.0
        lam = np.logspace(0.0, -p, n) * np.ones((nb, 1))
        return R._from_spectrum(rng, lam)
    if name == 'graded':                               # D A D, D = diag(2^k), k in [-8, 8]
        d = 2.0 ** rng.integers(-8, 9, (nb, n))
        return _wishart(rng, nb, n) * d[:, :, None] * d[:, None, :]
    if name == 'isotropic':                            # I + 1e-3 E
        e = rng.standard_normal((nb, n, n))
        return np.eye(n) + 1e-3 * (e + e.swapaxes(-1, -2)) / 2
    if name == 'equicorrelated':                       # (1 - rho) I + rho 1 1^T, rho up to 0.999
        rho = rng.uniform(0.0, 0.999, (nb, 1, 1))
        rho[-1] = 0.999
        return (1 - rho) * np.eye(n) + rho * np.ones((n, n))
    if name == 'scaled':                               # Wishart times 2^+-40 / 2^+-400
        e = 40 if dn == 'f32' else 400
        return _wishart(rng, nb, n) * 2.0 ** (e * rng.choice([-1.0, 1.0], (nb, 1, 1)))
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def batch(dn, n, nb=NB):
    """(compact records, vectors, cotangents of a scalar, {cell: slice}) of the dtype, read-only"""
    rng = np.random.default_rng(4000 + 10 * n + (dn == 'f64'))
    per = nb // len(CELLS)
    parts, cells, at = [], {}, 0
    for k, c in enumerate(CELLS):
        m = per if k + 1 < len(CELLS) else nb - at
        parts.append(cell(c, dn, rng, m, n))
        cells[c] = slice(at, at + m)
        at += m
    comp = R.pack(np.concatenate(parts)).astype(NP[dn])
    vec = rng.standard_normal((nb, n)).astype(NP[dn])
    g = rng.standard_normal(nb).astype(NP[dn])
    for x in (comp, vec, g):
        x.setflags(write=False)
    return comp, vec, g, cells


def bad_records(dn, n):
    """the bad cell: one negative eigenvalue, an exactly singular integer matrix ([[1, 1], [1, 1]] embedded: a pivot
    that is exactly 0), a NaN entry, an inf entry (on the diagonal, where only the entry test can see it)"""
    rng = np.random.default_rng(77 + n)
    lam = np.ones((1, n))
    lam[0, -1] = -0.5
    neg = R._from_spectrum(rng, lam)[0] if n > 1 else np.array([[-0.5]])
    sing = np.eye(n)
    if n > 1:
        sing[:2, :2] = 1.0
    else:
        sing[0, 0] = 0.0
    nan = _wishart(rng, 1, n)[0]
    nan[n - 1, 0] = nan[0, n - 1] = np.nan
    inf = _wishart(rng, 1, n)[0]
    inf[0, 0] = np.inf
    return R.pack(np.stack([neg, sing, nan, inf])).astype(NP[dn])


def judged(dn, n, comp):
    """kappa_2(D^-1 A D^-1) n eps <= 1/16 per record, D = sqrt diag A"""
    a = R.unpack(np.asarray(comp, np.float64), n)
    d = np.sqrt(np.diagonal(a, axis1=1, axis2=2))
    return np.linalg.cond(a / d[:, :, None] / d[:, None, :]) * n * R.eps_of(dn) <= 1.0 / 16


# ------------------------------------------------------------------------------------------------ plain routines
def chol_any(a):
    """batched lower Cholesky factor in the precision of `a`, from the definition"""
    nb, n, _ = a.shape
    l = np.zeros_like(a)
    for j in range(n):
        d = a[:, j, j].copy()
        for k in range(j):
            d = d - l[:, j, k] * l[:, j, k]
        with np.errstate(invalid='ignore'):
            l[:, j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            s = a[:, i, j].copy()
            for k in range(j):
                s = s - l[:, i, k] * l[:, j, k]
            with np.errstate(all='ignore'):
                l[:, i, j] = s / l[:, j, j]
    return l


def solve_lower(l, v):
    """L^-1 v by forward substitution in the precision of the arguments; v: (nb, n) or (nb, n, m)"""
    y = np.zeros_like(v)
    n = l.shape[-1]
    for i in range(n):
        s = v[:, i].copy()
        for k in range(i):
            s = s - (l[:, i, k] * y[:, k].T).T
        y[:, i] = (s.T / l[:, i, i]).T
    return y


def solve_upper(u, v):
    """U^-1 v by back substitution"""
    x = np.zeros_like(v)
    n = u.shape[-1]
    for i in range(n - 1, -1, -1):
        s = v[:, i].copy()
        for k in range(i + 1, n):
            s = s - (u[:, i, k] * x[:, k].T).T
        x[:, i] = (s.T / u[:, i, i]).T
    return x


def _mm(a, b):
    return np.einsum('bij,bjk->bik', a, b)


def _mv(a, v):
    return np.einsum('bij,bj->bi', a, v)


def plain(dn, comp, vec):
    """every forward result from the plain routines in the WORKING precision (no fused operations)"""
    T = NP[dn]
    n = vec.shape[-1]
    a = R.unpack(np.asarray(comp, T), n)
    v = np.asarray(vec, T)
    l = chol_any(a)
    lt = l.swapaxes(-1, -2)
    y = solve_lower(l, v)
    q = (y * y).sum(-1, dtype=T)
    logdet = (T(2) * np.log(np.diagonal(l, axis1=1, axis2=2))).sum(-1, dtype=T)
    return {'factor': R.pack(lt), 'L': _mv(l, v), 'LT': _mv(lt, v), 'Linv': y, 'LTinv': solve_upper(lt, v),
            'logdet': logdet, 'maha': q, 'maha_sqrt': np.sqrt(q),
            'logpdf': (T(-0.5) * (T(n) * T(LOG_2PI) + logdet + q)).astype(T)}


# ------------------------------------------------------------------------------------------------ the model
def model(dn, comp, vec, g):
    """the high-precision quantities of compact records of dtype dn, vectors and scalar cotangents"""
    hp = HP[dn]
    n = vec.shape[-1]
    a = R.unpack(np.asarray(comp).astype(hp), n)
    v = np.asarray(vec).astype(hp)
    g = np.asarray(g).astype(hp)
    l = chol_any(a)
    lt = l.swapaxes(-1, -2)
    eye = np.broadcast_to(np.eye(n, dtype=hp), a.shape)
    linv = solve_lower(l, eye.copy())
    linvt = linv.swapaxes(-1, -2)
    ainv = _mm(linvt, linv)
    P = _mm(np.abs(l), np.abs(lt))
    y = _mv(linv, v)
    w = _mv(linvt, y)
    q = (y * y).sum(-1)
    d = np.sqrt(q)
    logdiag = np.log(np.diagonal(l, axis1=1, axis2=2))
    return dict(n=n, a=a, v=v, g=g, l=l, linv=linv, ainv=ainv, P=P, y=y, w=w, q=q, d=d, logdet=2 * logdiag.sum(-1),
                abslog=np.abs(logdiag).sum(-1), ltv=_mv(lt, v), lv=_mv(l, v), x=_mv(linvt, v))


def _ratio(err, bound):
    """max over the components of a record of err / bound; a zero bound asks for a zero error"""
    err = np.asarray(err, np.float64).reshape(len(err), -1)
    bound = np.asarray(bound, np.float64).reshape(len(bound), -1)
    with np.errstate(all='ignore'):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(err), np.inf, r)
    return r.max(-1)


def _bounds(dn, m):
    """the forward bounds of the scalars (logdet, maha, maha_sqrt, logpdf) per record"""
    gm = gamma(dn, m['n'])
    aw, ay = np.abs(m['w']), np.abs(m['y'])
    b_logdet = gm * (np.abs(m['ainv']) * m['P']).sum((-1, -2)) + 2 * gm * m['abslog']
    b_maha = gm * ((aw * _mv(m['P'], aw)).sum(-1) + 2 * (aw * _mv(np.abs(m['l']), ay)).sum(-1) + m['q'])
    with np.errstate(all='ignore'):
        b_sqrt = np.where(m['d'] > 0, b_maha / (2 * m['d']), 0)
    return {'logdet': b_logdet, 'maha': b_maha, 'maha_sqrt': b_sqrt, 'logpdf': (b_logdet + b_maha) / 2}


def forward_ratio(dn, m, op, got):
    """per record: the largest error of `got` (the dtype's result of `op`) over its bound"""
    hp = HP[dn]
    n = m['n']
    gm = gamma(dn, n)
    got = np.asarray(got).astype(hp)
    al, alinv = np.abs(m['l']), np.abs(m['linv'])
    alt, alinvt = al.swapaxes(-1, -2), alinv.swapaxes(-1, -2)
    if op == 'factor':
        lh = np.tril(R.unpack(got, n))
        return _ratio(np.abs(m['a'] - _mm(lh, lh.swapaxes(-1, -2))), gm * m['P'])
    if op in APPLY:
        dl = gm * _mm(al, _mm(alinv, _mm(m['P'], alinvt)))          # |dL|, lower part and more
        dlt = dl.swapaxes(-1, -2)
        av = np.abs(m['v'])
        if op == 'L':
            want, bound = m['lv'], gm * _mv(al, av) + _mv(dl, av)
        elif op == 'LT':
            want, bound = m['ltv'], gm * _mv(alt, av) + _mv(dlt, av)
        elif op == 'Linv':
            ay = np.abs(m['y'])
            want, bound = m['y'], _mv(alinv, _mv(dl, ay)) + gm * _mv(alinv, _mv(al, ay))
        else:
            ax = np.abs(m['x'])
            want, bound = m['x'], _mv(alinvt, _mv(dlt, ax)) + gm * _mv(alinvt, _mv(alt, ax))
        return _ratio(np.abs(got - want), bound)
    want = {'logdet': m['logdet'], 'maha': m['q'], 'maha_sqrt': m['d'],
            'logpdf': -(n * hp(LOG_2PI) + m['logdet'] + m['q']) / 2}[op]
    return _ratio(np.abs(got - want), _bounds(dn, m)[op])


def backward_ratio(dn, m, op, got):
    """per record: the largest error of the packed gradient [K | n] (logdet: K) of `op` over its bound"""
    hp = HP[dn]
    n = m['n']
    K = n * (n + 1) // 2
    gm3 = 3 * gamma(dn, n)
    got = np.asarray(got).astype(hp)
    S_got = R.unpack(got[:, :K], n, off=0.5)
    g, ag = m['g'][:, None, None], np.abs(m['g'])[:, None, None]
    ainv, aainv, w, aw = m['ainv'], np.abs(m['ainv']), m['w'], np.abs(m['w'])
    d_ainv = gm3 * _mm(aainv, _mm(m['P'], aainv))
    d_w = gm3 * _mv(aainv, _mv(m['P'], aw))
    ww = w[:, :, None] * w[:, None, :]
    aww = aw[:, :, None] * aw[:, None, :]
    d_ww = d_w[:, :, None] * aw[:, None, :] + aw[:, :, None] * d_w[:, None, :]
    if op == 'logdet':
        return _ratio(np.abs(S_got - g * ainv), ag * d_ainv)
    gv_got = got[:, K:]
    if op == 'maha':
        S, bS = -g * ww, ag * d_ww
        gv, bv = 2 * g[:, :, 0] * w, 2 * ag[:, :, 0] * d_w
    elif op == 'maha_sqrt':
        d = m['d']
        with np.errstate(all='ignore'):
            c = np.where(d > 0, m['g'] / (2 * d), 0)
            d_d = _bounds(dn, m)['maha_sqrt']
            d_c = np.where(d > 0, np.abs(m['g']) * d_d / (2 * d * d), 0)
        c3, ac3, dc3 = c[:, None, None], np.abs(c)[:, None, None], d_c[:, None, None]
        S, bS = -c3 * ww, dc3 * aww + ac3 * d_ww
        gv, bv = 2 * c3[:, :, 0] * w, 2 * (dc3[:, :, 0] * aw + ac3[:, :, 0] * d_w)
    else:
        S, bS = -g * (ainv - ww) / 2, ag * (d_ainv + d_ww) / 2
        gv, bv = -g[:, :, 0] * w, ag[:, :, 0] * d_w
    return np.maximum(_ratio(np.abs(S_got - S), bS), _ratio(np.abs(gv_got - gv), bv))


@functools.lru_cache(maxsize=None)
def truth(dn, n):
    """model of batch(dn, n); computed once"""
    comp, vec, g, _ = batch(dn, n)
    return model(dn, comp, vec, g)


def worst(r, cells):
    return {c: float(r[sl].max()) for c, sl in cells.items()}
