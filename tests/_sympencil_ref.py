"""Reference model of the two-matrix spectral functions of `sym` (`sym_pencil_funm` and its wrappers, `sym_geneigvals`,
`sym_dist`) and of their gradients, numpy only, in the high precision of tests/_symfun_ref.py (float32 is judged in
float64, float64 in numpy.longdouble, `high_ok` asserted by the callers).

Per record, A SPD and B symmetric:  A = V L V^T, W = V L^-1/2, Y = V L^1/2, C = W^T B W = Q M Q^T, X = W Q, Z = Y Q.
    pencil function     G = Z f(M) Z^T
    its gradient (B)    X [(Z^T Gbar Z) o F] X^T, F_kl = f[mu_k, mu_l] (divdiff_hp: quotient / midpoint series)
    eigenvalues         mu ascending;  squared distance d2 = sum log^2 mu
    gradients of d2     with respect to B: X diag(2 log mu / mu) X^T, with respect to A: -X diag(2 log mu) X^T

Bounds (spectral norms of the full matrices, Frobenius norm of the errors), eta = n eps cond(A) ||C||: how far C moves
under backward-stable decompositions of A and the rounded triple product.
    eigenvalue i   c (eta + n eps |mu_i|)
    d2             c (eta sum_i 2 |log mu_i| / mu_i + n eps d2) + n M2d (c eta)^2
    function       c ||A|| (L eta + n eps ||f(C)||), L = max |F_kl|; exp: n + max|mu| in place of n (in eta too)
    gradient (B)   c n eps cond(A) ||A^-1|| (M2 ||C|| + L) ||Gbar||, M2 = sup |f''| / 2 over the spectrum's interval
    gradients of d2  the same with f = log^2 for B: f' = 2 log(mu) / mu, f'' = 2 (1 - log mu) / mu^2 (L and M2 are the
                   suprema over [mu_min, mu_max]: the endpoints and the interior extrema at e and e^1.5); for A the
                   spectral function is h = mu f' = 2 log mu: L = max |2 log mu|, M2 ||C|| -> sup |h'| ||C|| = 2 cond(C)

Two completions of these first-order statements, both needed for a bound that can hold at all.  The first-order
bound of d2 vanishes at A = B (every log mu_i = 0) while the computed mu_i sit within c eta of 1, so d2 comes out as
O(eta^2): the bound carries the Taylor remainder of log^2, sup |f''| / 2 = M2d per eigenvalue times (c eta)^2.  The
gradient of the function with respect to B does not change when A and B are scaled jointly (G scales with them), but
||A^-1|| does: for the `scaled` family the bound is that of the pair divided by its power of two, an exact operation
(`scale` below; 1 for every other family).

The constant c.  The composition of single-matrix functions the parent commit already had
(nitorch_fastmath_amd/_sympencil.py on CPU tensors, in the working dtype) was run against this model on every family
and order of tests/test_sympencil_host.py; its worst ratio to the bounds above with c = 1 is R_REF below, and
c = max(16, 2 R_REF rounded up to a power of two): 16 is the project's constant, the factor 2 is for the kernels' fast
sweeps and fma contraction.  R_REF is measured by `python tests/_sympencil_ref.py`.
"""
import functools
import math
import numpy as np
import _symfun_ref as R

NP, HP = R.NP, R.HP
FUNCS = ('exp', 'log', 'sqrt', 'rsqrt', 'pow')
POW_P = 0.3
FAMILIES = ('normal', 'graded', 'iso_base', 'equal', 'multiple', 'commuting', 'cluster', 'rank1', 'scaled',
            'indefinite')
PER = 43          # records per family in the host batches (387 records: several tiles and a ragged tail); the host tests
#                   run the longdouble model and the CPU composition on every family, order and function
PER_GPU = 301     # records per family in the batches of the GPU bound tests (2709 records)


def per_gpu(dn, n):
    """records per family of the GPU bound tests: PER_GPU, but PER for float64 at orders >= 6, where the longdouble
    Jacobi model of 2709 records takes 4 to 10 seconds per call and a test needs up to two calls"""
    return PER if (dn == 'f64' and n >= 6) else PER_GPU
R_REF = 14.1      # worst ratio of the composition to the bounds with c = 1 (measured 14.03: float64, n = 3, the
#                   gradient of exp on a `normal` pair; next 10.14, the gradient of pow on a `multiple` pair)
C = 32.0          # max(16, 2 R_REF rounded up to a power of two)


def fn_p(fn):
    return POW_P if fn == 'pow' else None


def families_of(fn):
    """exp takes any symmetric B (the `indefinite` family) and is not scale covariant; the others need B SPD"""
    if fn == 'exp':
        return tuple(f for f in FAMILIES if f != 'scaled')
    return tuple(f for f in FAMILIES if f != 'indefinite')


def _sqrt_spd(a):
    lam, v = np.linalg.eigh(a)
    return np.einsum('bik,bk,bjk->bij', v, np.sqrt(lam), v)


def _sym(a):
    return (a + a.swapaxes(-1, -2)) / 2


def family(name, dn, rng, nb, n):
    """nb float64 pairs (A SPD, B symmetric) of one family (rounded to the dtype by the caller)"""
    normal = lambda: R.family('normal', dn, rng, nb, n)          # noqa: E731
    if name == 'normal':
        return normal(), normal()
    if name == 'graded':          # cond(A) up to 1e3 / 1e8, ||C|| <= 1: eta below 1e-3
        dec = rng.uniform(0.0, 3.0 if dn == 'f32' else 8.0, (nb, 1))
        a = R._from_spectrum(rng, 2.0 * 10.0 ** (-dec * np.arange(n) / max(n - 1, 1)))
        s = _sqrt_spd(a)
        return a, _sym(s @ (normal() / 5.0) @ s)
    if name == 'iso_base':
        return np.eye(n) * rng.uniform(0.5, 4.0, (nb, 1, 1)), normal()
    if name == 'equal':
        a = normal()
        return a, a.copy()
    if name == 'multiple':
        a = normal()
        return a, a * rng.uniform(0.25, 4.0, (nb, 1, 1))
    if name == 'commuting':
        q = R._orth(rng, nb, n)
        mk = lambda: _sym(np.einsum('bij,bj,bkj->bik', q, rng.uniform(0.5, 5.0, (nb, n)), q))          # noqa: E731
        return mk(), mk()
    if name == 'cluster':          # mu = 1 +- 1e-5 / 1e-11
        a = normal()
        s = _sqrt_spd(a)
        d = 1e-5 if dn == 'f32' else 1e-11
        return a, _sym(s @ R._from_spectrum(rng, 1.0 + d * rng.uniform(-1.0, 1.0, (nb, n))) @ s)
    if name == 'rank1':
        a = normal()
        v = rng.standard_normal((nb, n))
        return a, a + v[:, :, None] * v[:, None, :]
    if name == 'scaled':          # both operands times 2^+-40 / 2^+-300
        e = 40 if dn == 'f32' else 300
        s = 2.0 ** (e * rng.choice([-1.0, 1.0], (nb, 1, 1)))
        return normal() * s, normal() * s
    if name == 'indefinite':          # for exp: ||C|| <= 20, eigenvalues of both signs
        a = normal()
        s = _sqrt_spd(a)
        return a, _sym(s @ R._from_spectrum(rng, rng.uniform(-20.0, 20.0, (nb, n))) @ s)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def batch(dn, n, fn, per=PER):
    """(compact A, compact B of the dtype, {family: slice}): every family of `fn` in one batch"""
    rng = np.random.default_rng(7000 * n + 10 * FUNCS.index(fn) + (dn == 'f64'))
    pa, pb, cells, at = [], [], {}, 0
    for f in families_of(fn):
        a, b = family(f, dn, rng, per, n)
        pa.append(a)
        pb.append(b)
        cells[f] = slice(at, at + per)
        at += per
    ca, cb = R.pack(np.concatenate(pa)).astype(NP[dn]), R.pack(np.concatenate(pb)).astype(NP[dn])
    if 'equal' in cells:          # still equal after the rounding
        cb[cells['equal']] = ca[cells['equal']]
    ca.setflags(write=False)
    cb.setflags(write=False)
    return ca, cb, cells


def _eigh(a):
    if a.dtype == np.float64:
        return np.linalg.eigh(a)
    return R.jacobi_eigh(a)


def _mid(lo, hi, at, val):
    """val where lo < at < hi, else 0"""
    return np.where((lo < at) & (at < hi), val, 0.0)


def model(dn, fn, ca, cb, p=None, g=None):
    """the high-precision model for compact pairs of dtype dn (and a compact cotangent g of the function).
    dict: G, SB (full symmetric; SB None without g), mu, d2, gA, gB (full gradients of d2 for the cotangent 1) and the
    numbers of the bounds (float64)."""
    hp = HP[dn]
    n = int((math.isqrt(1 + 8 * ca.shape[-1]) - 1) // 2)
    A, B = R.unpack(np.asarray(ca), n).astype(hp), R.unpack(np.asarray(cb), n).astype(hp)
    lam, V = _eigh(A)
    W, Y = V / np.sqrt(lam)[:, None, :], V * np.sqrt(lam)[:, None, :]
    Cm = _sym(np.einsum('bik,bij,bjl->bkl', W, B, W))
    mu, Q = _eigh(Cm)
    X, Z = W @ Q, Y @ Q
    out = dict(n=n, mu=mu)
    lo, hi = mu.min(1), mu.max(1)
    f64 = lambda x: np.asarray(x, np.float64)          # noqa: E731
    out['kappa'], out['normA'], out['invA'] = f64(lam.max(1) / lam.min(1)), f64(lam.max(1)), f64(1 / lam.min(1))
    # the power of two of the `scaled` family (1 elsewhere: ||A|| is within [2^-10, 2^3] there)
    e = 40 if dn == 'f32' else 300
    out['scale'] = np.where(out['normA'] > 2.0 ** (e / 2), 2.0 ** e, np.where(out['normA'] < 2.0 ** (-e / 2), 2.0 ** -e, 1.0))
    out['normC'], out['mu_max'] = f64(np.abs(mu).max(1)), f64(np.abs(mu).max(1))
    with np.errstate(all='ignore'):
        if fn is not None:
            f = R._deriv(fn, p, 0, mu)
            out['G'] = np.einsum('bik,bk,bjk->bij', Z, f, Z)
            a2, b2 = np.broadcast_arrays(mu[:, :, None], mu[:, None, :])
            F = R.divdiff_hp(fn, p, a2, b2)
            out['L'], out['normF'] = f64(np.abs(F).max((1, 2))), f64(np.abs(f).max(1))
            out['M2'] = f64(np.maximum(np.abs(R._deriv(fn, p, 2, lo)), np.abs(R._deriv(fn, p, 2, hi)))) / 2
            out['SB'] = None
            if g is not None:
                Gb = R.unpack(np.asarray(g).astype(hp), n, off=0.5)
                H = np.einsum('bik,bij,bjl->bkl', Z, Gb, Z) * F
                out['SB'] = np.einsum('bik,bkl,bjl->bij', X, H, X)
        if fn != 'exp':          # the distance: B SPD
            lg = np.log(mu)
            out['d2'] = (lg * lg).sum(1)
            out['gB'] = np.einsum('bik,bk,bjk->bij', X, 2 * lg / mu, X)
            out['gA'] = -np.einsum('bik,bk,bjk->bij', X, 2 * lg, X)
            out['sum_fp'] = f64((2 * np.abs(lg) / mu).sum(1))
            fp = lambda x: np.abs(2 * np.log(x) / x)          # noqa: E731
            fpp = lambda x: np.abs(2 * (1 - np.log(x)) / (x * x))          # noqa: E731
            lo64, hi64 = f64(lo), f64(hi)
            out['Ld'] = np.maximum(np.maximum(fp(lo64), fp(hi64)), _mid(lo64, hi64, math.e, 2 / math.e))
            out['M2d'] = np.maximum(np.maximum(fpp(lo64), fpp(hi64)), _mid(lo64, hi64, math.e ** 1.5, math.e ** -3)) / 2
            out['Lh'] = np.maximum(np.abs(2 * np.log(lo64)), np.abs(2 * np.log(hi64)))
            out['M2h_normC'] = 2 * hi64 / lo64
    return out


def cotangent(dn, n, nb, seed=17):
    rng = np.random.default_rng(seed + n)
    g = rng.standard_normal((nb, n * (n + 1) // 2)).astype(NP[dn])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def truth(dn, n, fn, per=PER):
    ca, cb, _ = batch(dn, n, fn, per)
    return model(dn, fn, ca, cb, fn_p(fn), cotangent(dn, n, len(ca)))


# ------------------------------------------------------------------------------------------------ ratios (the bar is C)
def _nfac(fn, mod):
    return mod['n'] + (mod['mu_max'] if fn == 'exp' else 0.0)


def eig_ratio(dn, mod, got):
    eps, n = R.eps_of(dn), mod['n']
    eta = n * eps * mod['kappa'] * mod['normC']
    err = np.abs(np.asarray(got).astype(HP[dn]) - mod['mu']).astype(np.float64)
    return (err / (eta[:, None] + n * eps * np.abs(mod['mu']).astype(np.float64))).max(1)


def dist2_bound(dn, mod):
    """the bound of d2 divided by C: the first-order terms and the remainder n M2d (C eta)^2 over C"""
    eps, n = R.eps_of(dn), mod['n']
    eta = n * eps * mod['kappa'] * mod['normC']
    return eta * mod['sum_fp'] + n * eps * mod['d2'].astype(np.float64) + C * n * mod['M2d'] * eta * eta


def dist2_ratio(dn, mod, got):
    err = np.abs(np.asarray(got).astype(HP[dn]) - mod['d2']).astype(np.float64)
    return err / dist2_bound(dn, mod)


def fun_bound(dn, fn, mod):
    """the forward bound with c = 1"""
    nf, eps = _nfac(fn, mod), R.eps_of(dn)
    return mod['normA'] * (mod['L'] * nf * eps * mod['kappa'] * mod['normC'] + nf * eps * mod['normF'])


def fun_ratio(dn, fn, mod, got):
    err = R._fro(R.unpack(np.asarray(got).astype(HP[dn]), mod['n']) - mod['G'])
    return err / fun_bound(dn, fn, mod)


def grad_ratio(dn, fn, mod, g, got, want=None, unit_scale=False):
    """gradient with respect to B of the function (want: another full symmetric target of the same bound).
    unit_scale: ||A^-1|| of the pair divided by the power of two next to ||A||, for every record.  The gradient does
    not change under a joint scaling of the pair while ||A^-1|| does, so the bound as stated falls below the rounding
    of the result itself once ||A|| is well above 1; the tests use this form where the issue sets no bound of its own:
    the gradient with respect to the base through the swap identity, whose base is B (up to 4 A in `multiple`)."""
    n, eps = mod['n'], R.eps_of(dn)
    err = R._fro(R.unpack(np.asarray(got).astype(HP[dn]), n, off=0.5) - (mod['SB'] if want is None else want))
    G = R._fro(R.unpack(np.asarray(g).astype(np.float64), n, off=0.5))
    inv = mod['invA'] * (2.0 ** np.floor(np.log2(mod['normA'])) if unit_scale else mod['scale'])
    return err / (_nfac(fn, mod) * eps * mod['kappa'] * inv * (mod['M2'] * mod['normC'] + mod['L']) * G)


def dist_grad_bounds(dn, mod):
    """(bound of the gradient with respect to A, with respect to B) of d2 for the cotangent 1, c = 1"""
    n, eps = mod['n'], R.eps_of(dn)
    pre = n * eps * mod['kappa'] * mod['invA']
    return pre * (mod['M2h_normC'] + mod['Lh']), pre * (mod['M2d'] * mod['normC'] + mod['Ld'])


def dist_grad_ratios(dn, mod, gA, gB):
    n = mod['n']
    ba, bb = dist_grad_bounds(dn, mod)
    ea = R._fro(R.unpack(np.asarray(gA).astype(HP[dn]), n, off=0.5) - mod['gA'])
    eb = R._fro(R.unpack(np.asarray(gB).astype(HP[dn]), n, off=0.5) - mod['gB'])
    return ea / ba, eb / bb


# ------------------------------------------------------------------------------------------------ the constant
def composition(dn, fn, ca, cb, g):
    """the composition route on CPU tensors of the working dtype: (G, SB, mu, d2, gA, gB) as numpy arrays"""
    import torch
    from nitorch_fastmath_amd import _sympencil as P
    from nitorch_fastmath_amd import _symfun
    a, b = torch.from_numpy(np.array(ca)), torch.from_numpy(np.array(cb)).requires_grad_(True)
    y = P.pencil_funm(a, b, _symfun_code(fn), fn_p(fn))
    (sb,) = torch.autograd.grad(y, b, torch.from_numpy(np.array(g)))
    res = [y.detach().numpy(), sb.numpy(), P.geneigvals(a, b).detach().numpy()]
    if fn != 'exp':
        a = a.requires_grad_(True)
        d2 = P.dist(a, b, squared=True)
        ga, gb = torch.autograd.grad(d2.sum(), (a, b))
        res += [d2.detach().numpy(), ga.numpy(), gb.numpy()]
    return res


def _symfun_code(fn):
    return R.FUNCS.index(fn)


def composition_ratios(dn, n, fn):
    """{quantity: per-record ratio of the composition to the bounds with c = 1}"""
    ca, cb, _ = batch(dn, n, fn)
    g = cotangent(dn, n, len(ca))
    mod = truth(dn, n, fn)
    res = composition(dn, fn, ca, cb, g)
    out = {'fun': fun_ratio(dn, fn, mod, res[0]), 'grad': grad_ratio(dn, fn, mod, g, res[1]),
           'eig': eig_ratio(dn, mod, res[2])}
    if fn != 'exp':
        out['d2'] = dist2_ratio(dn, mod, res[3])
        out['gA'], out['gB'] = dist_grad_ratios(dn, mod, res[4], res[5])
    return out


if __name__ == '__main__':
    worst = 0.0
    for dn in ('f32', 'f64'):
        for n in (1, 2, 3, 4, 6, 8, 9):
            for fn in FUNCS:
                _, _, cells = batch(dn, n, fn)
                for q, r in composition_ratios(dn, n, fn).items():
                    k = int(np.nanargmax(r))
                    fam = [f for f, sl in cells.items() if sl.start <= k < sl.stop][0]
                    print(f'{dn} n={n} {fn} {q}: {np.nanmax(r):.2f} ({fam})', 'NAN' if np.isnan(r).any() else '')
                    worst = max(worst, float(np.nanmax(r)))
    print('R_REF', worst)
