"""Inputs, truths and bounds shared by tests/test_polar_host.py and tests/test_gpu_polar.py (`batched.batchsvdvals`,
`batchsvd`, `batchpolar` and their gradients).

Families (built from U diag(sigma) V^T in float64 and rounded to the dtype, `_svd_ref.from_sigma`): normal; graded
(sigma log-spaced to cond 1e3 / 1e6); repeated (a scaled orthogonal matrix); cluster (sigma = 1 + 2^-k u); negdet;
scaled (by 2^+-40 / 2^+-300); rankdef (integer-valued records with duplicated rows: ranks n - 1, n - 1, 1 and 0 in
turn).

Truths.  tests/golden/polar.npz (tests/golden/make_golden_polar.py, mpmath at 50 digits) holds NFIX records per
(dtype, order, family) with S, R, P and the gradients for the cotangents of `cotangents()`.  A batch of `batch()`
starts with those records and goes on with NB - 21 more of the same families.  float32 results are judged on the whole
batch against numpy's float64 SVD of the rounded input; float64 results against the fixture on its records, and on
every record by the bounds that need no truth (residual, orthogonality, symmetry, definiteness, order).

Bounds, per record, Frobenius norms, C = 16 (the constant `_symfun_ref.C` allows an in-register Jacobi decomposition
plus recomposition), eps of the dtype:
    residual       |A - U S Vh|, |A - R P|          <= C n eps |A|
    orthogonality  |U^T U - I|, |Vh Vh^T - I|, |R^T R - I|  <= C n eps
    values         max_i |s^_i - s_i|              <= C n eps s_1                        (Weyl)
    stretch        |P^ - P|                         <= C n eps sqrt(2) |A|_2,  P^ exactly symmetric,
                   lambda_min(P^)                   >= -C n eps |A|_2
    rotation       |R^ - R|                         <= C n eps (1 + 2 |A|_2 / g),  g = s_{n-1} + s_n (2 s_1 for n = 1):
                   the condition number of the orthogonal polar factor; not asked of rank-deficient records
    polar gradient |dA^ - dA| <= 2 err_ref + C n eps [(2 / g + 2 |A|_2 / g^2) |gR| + (2 + 2 |A|_2 / g) |gP|]
                   err_ref: the error, against the same truth, of the closed form evaluated from torch's CPU SVD in the
                   same dtype (`_polar.polar_backward` on CPU tensors); asked of the full-rank families (`grad_ratios`)
    values gradient |dA^ - U diag(g) Vh| <= 2 err_ref + C n eps (1 + 2 |A|_2 / d) |g|,  d = min_{i != j} |s_i - s_j|:
                   the outer products u_i v_i^T move by eps |A|_2 / d under a backward error eps |A| (Wedin); asked of
                   the families with separated singular values (normal, graded, negdet, scaled)
"""
import functools
import os
import numpy as np
from _svd_ref import NP, TT, CODE, from_sigma          # noqa: F401

C = 16.0
ORDERS = (1, 2, 3, 4, 6, 8)
FAMILIES = ('normal', 'graded', 'repeated', 'cluster', 'negdet', 'scaled', 'rankdef')
SEPARATED = ('normal', 'graded', 'negdet', 'scaled')
NFIX = 3                     # fixture records per (dtype, order, family)
NB = 2 * 512 + 176           # two full tiles of the largest tile of the frame and a ragged tail
VALS, FULL, POLAR, BWD = range(4)
HI = np.longdouble
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'polar.npz')


def eps_of(dn):
    return float(np.finfo(NP[dn]).eps)


def _seed(fam, n, dn, extra):
    return 7000 + 1000 * FAMILIES.index(fam) + 10 * n + (dn == 'f64') + 100000 * extra


def _rankdef(n, count, rng):
    out = np.zeros((count, n, n))
    for k in range(count):
        kind = k % 4
        if kind == 3:
            continue
        while True:
            m = rng.integers(-4, 5, (n, n)).astype(np.float64)
            if kind == 2:
                mult = rng.integers(1, 4, n) * rng.choice([-1, 1], n)
                m = mult[:, None] * m[0][None, :]
                want = 1
            else:
                if n > 1:
                    m[n - 1] = m[0]
                else:
                    m[:] = 0
                want = n - 1
            if np.linalg.matrix_rank(m) == min(want, n):
                break
        out[k] = m
    return out


def family(fam, n, count, dn, extra=0):
    """`count` records (count, n, n) of the family in the dtype; `extra` selects another draw"""
    seed = _seed(fam, n, dn, extra)
    rng = np.random.default_rng(seed)
    if fam == 'normal':
        return rng.standard_normal((count, n, n)).astype(NP[dn])
    if fam == 'rankdef':
        return _rankdef(n, count, rng).astype(NP[dn])
    if fam == 'graded':
        cond = 1e3 if dn == 'f32' else 1e6
        sigma = np.logspace(0.0, -np.log10(cond), n) if n > 1 else np.ones(1)
        sigma = sigma[None, :] * rng.uniform(0.5, 2.0, (count, 1))
    elif fam == 'repeated':
        sigma = np.repeat(rng.uniform(0.5, 2.0, (count, 1)), n, 1)
    elif fam == 'cluster':
        k = 1 + (np.arange(count) % (20 if dn == 'f32' else 48))
        sigma = 1.0 + np.ldexp(rng.uniform(0.0, 1.0, (count, n)), -k[:, None])
    else:
        sigma = np.sort(rng.uniform(0.2, 2.0, (count, n)), -1)[:, ::-1]
    a = from_sigma(count, n, n, sigma, dn, seed + 1).astype(np.float64)
    if fam == 'negdet':
        a[:, 0, :] *= np.where(np.linalg.det(a) > 0, -1.0, 1.0)[:, None]
    if fam == 'scaled':
        e = 40 if dn == 'f32' else 300
        a = np.ldexp(a, np.where(np.arange(count) % 2 == 0, e, -e)[:, None, None])
    return a.astype(NP[dn])


def cotangents(n, count, dn, fam):
    """(gR, gP, gS) of the fixture records: standard normal, in the dtype"""
    rng = np.random.default_rng(_seed(fam, n, dn, 7))
    return (rng.standard_normal((count, n, n)).astype(NP[dn]), rng.standard_normal((count, n, n)).astype(NP[dn]),
            rng.standard_normal((count, n)).astype(NP[dn]))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def fix(dn, n, fam, what):
    return fixture()[f'{dn}_{n}_{fam}_{what}']


@functools.lru_cache(maxsize=None)
def batch(dn, n):
    """(a (NB, n, n), family index of every record): the fixture records of every family first (family-major), then
    more of the same families.  Read-only."""
    nfix = NFIX * len(FAMILIES)
    more = (NB - nfix + len(FAMILIES) - 1) // len(FAMILIES)
    a = [family(f, n, NFIX, dn) for f in FAMILIES] + [family(f, n, more, dn, 1) for f in FAMILIES]
    fam = [np.full(NFIX, i) for i in range(len(FAMILIES))] + [np.full(more, i) for i in range(len(FAMILIES))]
    a, fam = np.concatenate(a)[:NB], np.concatenate(fam)[:NB]
    a.setflags(write=False)
    fam.setflags(write=False)
    return a, fam


def fixture_truth(dn, n, what):
    """the fixture's truths in the order of the first records of `batch`"""
    return np.concatenate([fix(dn, n, f, what) for f in FAMILIES])


def fixture_cotangents(dn, n):
    parts = [cotangents(n, NFIX, dn, f) for f in FAMILIES]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


# ------------------------------------------------------------------------------------------------ norms and ratios
def fro(x):
    x = np.asarray(x, HI)
    return np.sqrt((x * x).sum((-2, -1)))


def _ratio(err, bound):
    """err / bound per record; a zero bound asks for a zero error; a non-finite error counts as inf"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(err), r, np.inf)


def _eye(n):
    return np.eye(n, dtype=HI)


def _mm(*ms):
    out = np.asarray(ms[0], HI)
    for m in ms[1:]:
        out = np.einsum('...ij,...jk->...ik', out, np.asarray(m, HI))
    return out


def _t(x):
    return np.swapaxes(x, -1, -2)


def truth64(a):
    """numpy's float64 SVD of the input as rounded: S, R = U Vh, P = Vh^T S Vh (the float32 truth)"""
    a64 = np.asarray(a, np.float64)
    u, s, vh = np.linalg.svd(a64)
    return s, u @ vh, _t(vh) @ (s[..., :, None] * vh)


def gap_sum(s):
    s = np.asarray(s, np.float64)
    return 2.0 * s[..., 0] if s.shape[-1] == 1 else s[..., -1] + s[..., -2]


def svd_ratios(dn, a, U, S, Vh):
    n, e = a.shape[-1], eps_of(dn)
    aS = np.asarray(S, HI)
    res = fro(np.asarray(a, HI) - _mm(np.asarray(U, HI) * aS[..., None, :], Vh))
    out = {'residual': _ratio(res, C * n * e * fro(a)),
           'orth U': _ratio(fro(_mm(_t(U), U) - _eye(n)), C * n * e),
           'orth Vh': _ratio(fro(_mm(Vh, _t(Vh)) - _eye(n)), C * n * e)}
    return out


def ordered(S):
    S = np.asarray(S)
    return bool((S >= 0).all() and (S[..., :-1] >= S[..., 1:]).all() and np.isfinite(S).all())


def vals_ratio(dn, S, S_true):
    n = S.shape[-1]
    err = np.abs(np.asarray(S, HI) - np.asarray(S_true, HI)).max(-1)
    return _ratio(err, C * n * eps_of(dn) * np.asarray(S_true, np.float64)[..., 0])


def polar_self_ratios(dn, a, R, P, norm2):
    """the bounds that need no truth beyond |A|_2: orthogonality of R, |A - R P|, definiteness; and exact symmetry"""
    n, e = a.shape[-1], eps_of(dn)
    lam = np.linalg.eigvalsh(np.asarray(P, np.float64))[..., 0]
    out = {'orth R': _ratio(fro(_mm(_t(R), R) - _eye(n)), C * n * e),
           'A - R P': _ratio(fro(np.asarray(a, HI) - _mm(R, P)), C * n * e * fro(a)),
           'lambda_min': _ratio(np.maximum(-lam, 0.0), C * n * e * norm2)}
    return out, bool(np.array_equal(np.asarray(P), _t(np.asarray(P))))


def stretch_ratio(dn, P, P_true, norm2):
    n = P.shape[-1]
    return _ratio(fro(np.asarray(P, HI) - np.asarray(P_true, HI)), C * n * eps_of(dn) * np.sqrt(2.0) * norm2)


def rotation_ratio(dn, R, R_true, S_true):
    n = R.shape[-1]
    s = np.asarray(S_true, np.float64)
    with np.errstate(divide='ignore'):
        bound = C * n * eps_of(dn) * (1.0 + 2.0 * s[..., 0] / gap_sum(s))
    return _ratio(fro(np.asarray(R, HI) - np.asarray(R_true, HI)), bound)


def polar_grad_ratio(dn, ga, ga_true, ga_ref, S_true, gr, gp):
    n = ga.shape[-1]
    s = np.asarray(S_true, np.float64)
    g, a2 = gap_sum(s), s[..., 0]
    ngr = 0.0 if gr is None else np.asarray(fro(gr), np.float64)
    ngp = 0.0 if gp is None else np.asarray(fro(gp), np.float64)
    err_ref = np.asarray(fro(np.asarray(ga_ref, HI) - np.asarray(ga_true, HI)), np.float64)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        bound = 2.0 * err_ref + C * n * eps_of(dn) * ((2.0 / g + 2.0 * a2 / g ** 2) * ngr + (2.0 + 2.0 * a2 / g) * ngp)
    return _ratio(fro(np.asarray(ga, HI) - np.asarray(ga_true, HI)), bound)


def vals_grad_ratio(dn, ga, ga_true, ga_ref, S_true, gs):
    n = ga.shape[-1]
    s = np.asarray(S_true, np.float64)
    if n > 1:
        d = np.abs(s[..., :, None] - s[..., None, :]) + np.where(np.eye(n) > 0, np.inf, 0.0)
        d = d.min((-2, -1))
    else:
        d = np.full(s.shape[:-1], np.inf)
    err_ref = np.asarray(fro(np.asarray(ga_ref, HI) - np.asarray(ga_true, HI)), np.float64)
    ng = np.sqrt((np.asarray(gs, np.float64) ** 2).sum(-1))
    with np.errstate(divide='ignore'):
        bound = 2.0 * err_ref + C * n * eps_of(dn) * (1.0 + 2.0 * s[..., 0] / d) * ng
    return _ratio(fro(np.asarray(ga, HI) - np.asarray(ga_true, HI)), bound)


def report(what, ratios):
    """print the worst ratio of every bound (before anything is asserted) and return the largest"""
    worst = 0.0
    for k, v in ratios.items():
        v = np.asarray(v, np.float64)
        i = int(np.argmax(v)) if v.size else 0
        w = float(v[i]) if v.size else 0.0
        print(f'{what}: {k}: worst ratio {w:.3g} of 1 (= {w * C:.3g} n eps units), record {i}')
        worst = max(worst, w)
    return worst


# ------------------------------------------------------------------------------------------------ the host entry
def host(L, op, a, gr=None, gp=None):
    """nfm_polar_host on numpy records a (m, n, n): (packed result (m, ncomp), largest sweep count)"""
    a = np.ascontiguousarray(a)
    dn = 'f32' if a.dtype == np.float32 else 'f64'
    m, n = a.shape[0], a.shape[-1]
    ncomp = {VALS: n, FULL: n + 2 * n * n, POLAR: 2 * n * n, BWD: n * n}[op]
    out = np.empty((m, ncomp), a.dtype)
    gr = None if gr is None else np.ascontiguousarray(gr, a.dtype)
    gp = None if gp is None else np.ascontiguousarray(gp, a.dtype)
    rc = L.nfm_polar_host(CODE[dn], op, n, m, a.ctypes.data, None if gr is None else gr.ctypes.data,
                          None if gp is None else gp.ctypes.data, out.ctypes.data)
    assert rc >= 0, rc
    return out, rc


def split_full(out, n):
    m = out.shape[0]
    return (out[:, n:n + n * n].reshape(m, n, n), out[:, :n], out[:, n + n * n:].reshape(m, n, n))


def split_polar(out, n):
    m = out.shape[0]
    return out[:, :n * n].reshape(m, n, n), out[:, n * n:].reshape(m, n, n)


# ------------------------------------------------------------------------------------------------ whole-batch checks
def true_rank(S_true):
    s = np.asarray(S_true, np.float64)
    return (s > 1e-30 * np.maximum(s[..., :1], 1e-300)).sum(-1)


def forward_ratios(dn, n, S=None, svd=None, polar=None):
    """every forward bound on results for `batch(dn, n)` (numpy arrays; any of the three may be None): a dict of
    per-record ratios (bound = 1), and asserts what is not a ratio (finite, order, sign, symmetry)"""
    a, fam = batch(dn, n)
    nfix = NFIX * len(FAMILIES)
    norm2 = np.linalg.svd(np.asarray(a, np.float64), compute_uv=False)[:, 0]
    if dn == 'f32':
        St, Rt, Pt = truth64(a)
        sel = np.arange(len(a))
    else:
        St, Rt, Pt = (fixture_truth(dn, n, k) for k in ('S', 'R', 'P'))
        sel = np.arange(nfix)
    full = fam[sel] != FAMILIES.index('rankdef')
    out = {}
    if S is not None:
        assert ordered(S), 'S must be finite, non-negative and descending'
        out['values'] = vals_ratio(dn, S[sel], St)
    if svd is not None:
        U, S2, Vh = svd
        assert np.isfinite(U).all() and np.isfinite(Vh).all() and ordered(S2)
        out.update(svd_ratios(dn, a, U, S2, Vh))
        out['values (svd)'] = vals_ratio(dn, S2[sel], St)
    if polar is not None:
        R_, P_ = polar
        assert np.isfinite(R_).all() and np.isfinite(P_).all()
        ratios, sym = polar_self_ratios(dn, a, R_, P_, norm2)
        assert sym, 'P must have exactly equal mirrored entries'
        out.update(ratios)
        out['stretch'] = stretch_ratio(dn, P_[sel], Pt, norm2[sel])
        out['rotation'] = np.zeros(len(sel))          # (aligned with the records; rank-deficient ones are not asked)
        out['rotation'][full] = rotation_ratio(dn, R_[sel][full], Rt[full], St[full])
    return out


def grad_cases(dn, n):
    """the fixture records, their cotangents and truths, and the masks of the gradient tests:
    `diff`: R is differentiable (rank >= n - 1) -- held to the polar gradient bound;
    `sep`: singular values separated by construction -- held to the values gradient bound"""
    nfix = NFIX * len(FAMILIES)
    a, fam = batch(dn, n)
    a, fam = a[:nfix], fam[:nfix]
    gr, gp, gs = fixture_cotangents(dn, n)
    T = {k: fixture_truth(dn, n, k) for k in ('S', 'gaR', 'gaP', 'gaS')}
    assert np.array_equal(a, fixture_truth(dn, n, 'a')), 'the fixture is stale: run tests/golden/make_golden_polar.py'
    diff = true_rank(T['S']) >= n - 1
    sep = np.isin(fam, [FAMILIES.index(f) for f in SEPARATED])
    return a, fam, gr, gp, gs, T, diff, sep


def torch_ref_polar_grad(a, gr, gp):
    """the closed form from torch's CPU SVD in the dtype of a (err_ref of the gradient bound)"""
    import torch
    from nitorch_fastmath_amd import _polar
    t = lambda x: None if x is None else torch.from_numpy(np.array(x))          # noqa: E731
    return _polar.polar_backward(t(a), t(gr), t(gp)).numpy()


def torch_ref_vals_grad(a, gs):
    import torch
    from nitorch_fastmath_amd import _polar
    return _polar.svdvals_backward(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(gs))).numpy()


def grad_ratios(dn, n, ga_r=None, ga_p=None, ga_rp=None, ga_s=None):
    """the gradient bounds on results for the fixture records (numpy arrays, any may be None), and the NaN rule:
    where R is not differentiable a gradient with a non-zero gR is NaN throughout and the gP part is finite.
    The bound is asked of the full-rank families.  At an exactly singular record of rank n - 1 the decomposition that
    is returned is one of two branches (the sign of u_n v_n^T is free, and with it det R), and the gradient is that
    of the branch: kernel, torch and mpmath each pick their own, so such a record is only held to a finite result."""
    a, fam, gr, gp, gs, T, diff, sep = grad_cases(dn, n)
    full = fam != FAMILIES.index('rankdef')
    out = {}
    for name, got, r, p, tr in (('grad gR', ga_r, gr, None, T['gaR']), ('grad gP', ga_p, None, gp, T['gaP']),
                                ('grad gR+gP', ga_rp, gr, gp, T['gaR'] + T['gaP'])):
        if got is None:
            continue
        ref = torch_ref_polar_grad(a, r, p)
        sub = lambda x: None if x is None else x[full]          # noqa: E731
        out[name] = np.zeros(len(a))
        out[name][full] = polar_grad_ratio(dn, got[full], tr[full], ref[full], T['S'][full], sub(r), sub(p))
        assert np.isfinite(got[diff]).all(), 'finite wherever R is differentiable'
        if r is not None:
            assert np.isnan(got[~diff]).all(), 'rank <= n - 2 with a non-zero gR: the gradient record is NaN'
        else:
            assert np.isfinite(got[~diff]).all(), 'the gP part is finite at every rank'
    if ga_s is not None:
        assert np.isfinite(ga_s).all()
        ref = torch_ref_vals_grad(a, gs)
        out['grad gS'] = np.zeros(len(a))
        out['grad gS'][sep] = vals_grad_ratio(dn, ga_s[sep], T['gaS'][sep], ref[sep], T['S'][sep], gs[sep])
    return out
