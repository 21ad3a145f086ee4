"""Writes tests/golden/polar.npz: the truths of tests/_polar_ref.py's fixture records, computed with mpmath at 50
digits from the inputs as rounded to the dtype.  Per (dtype, order, family), NFIX records:
    a   the input (in the dtype)            S   singular values, descending
    R   U Vh (of no use for rankdef)         P   Vh^T diag(S) Vh
    gaR / gaP  the gradient of batchpolar for the cotangent gR alone / gP alone of `_polar_ref.cotangents`
    gaS        U diag(gS) Vh, the gradient of batchsvdvals (meaningful where the singular values are separated)
all truths rounded to float64.  The gradient form U X V^T, X_ij = ((B - B^T)_ij + 2 s_i C_ij) / (s_i + s_j), is itself
checked here against central differences at 50 digits on the small orders (`check_form`).

usage: python tests/golden/make_golden_polar.py        (needs mpmath; a few minutes)"""
import os
import sys
import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _polar_ref as R          # noqa: E402

mp.mp.dps = 50


def to_mp(x):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(x)])


def to_np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def decompose(A):
    """U, S (list, descending), Vh in mp; A = U diag(S) Vh"""
    U, S, Vh = mp.svd_r(A)
    return U, [S[i] for i in range(A.rows)], Vh


def polar(A):
    U, S, Vh = decompose(A)
    return U * Vh, Vh.T * mp.diag(S) * Vh


def polar_grad(A, gr, gp):
    """the closed form; a pair of zero singular values contributes by the kernels' rule (factor 1, no gR part)"""
    n = A.rows
    U, S, Vh = decompose(A)
    V = Vh.T
    B = U.T * gr * V if gr is not None else mp.zeros(n)
    C = Vh * ((gp + gp.T) / 2) * V if gp is not None else mp.zeros(n)
    tiny = mp.mpf(10) ** -40 * (S[0] if S[0] > 0 else 1)
    X = mp.zeros(n)
    for i in range(n):
        for j in range(n):
            if S[i] <= tiny and S[j] <= tiny:
                X[i, j] = C[i, j]
            else:
                X[i, j] = ((B[i, j] - B[j, i]) + 2 * S[i] * C[i, j]) / (S[i] + S[j])
    return U * X * Vh


def vals_grad(A, gs):
    U, S, Vh = decompose(A)
    return U * mp.diag([mp.mpf(float(g)) for g in gs]) * Vh


def check_form(A, gr, gp):
    """<gR, dR> + <gP, dP> by central differences at 50 digits against <polar_grad, dA> entry by entry"""
    n, h = A.rows, mp.mpf(10) ** -20
    G = polar_grad(A, gr, gp)
    worst = mp.mpf(0)
    for i in range(n):
        for j in range(n):
            E = mp.zeros(n)
            E[i, j] = h
            Rp, Pp = polar(A + E)
            Rm, Pm = polar(A - E)
            fd = sum(gr[k, l] * (Rp[k, l] - Rm[k, l]) + gp[k, l] * (Pp[k, l] - Pm[k, l])
                     for k in range(n) for l in range(n)) / (2 * h)
            worst = max(worst, abs(fd - G[i, j]))
    return worst


def main():
    out = {}
    for dn in ('f32', 'f64'):
        for n in R.ORDERS:
            for fam in R.FAMILIES:
                a = R.family(fam, n, R.NFIX, dn)
                gr, gp, gs = R.cotangents(n, R.NFIX, dn, fam)
                acc = {k: [] for k in ('S', 'R', 'P', 'gaR', 'gaP', 'gaS')}
                for k in range(R.NFIX):
                    A, GR, GP = to_mp(a[k]), to_mp(gr[k]), to_mp(gp[k])
                    U, S, Vh = decompose(A)
                    acc['S'].append([float(s) for s in S])
                    acc['R'].append(to_np(U * Vh))
                    acc['P'].append(to_np(Vh.T * mp.diag(S) * Vh))
                    acc['gaR'].append(to_np(polar_grad(A, GR, None)))
                    acc['gaP'].append(to_np(polar_grad(A, None, GP)))
                    acc['gaS'].append(to_np(vals_grad(A, gs[k])))
                    if n <= 3 and k == 0 and fam in ('normal', 'repeated', 'cluster', 'negdet'):
                        w = check_form(A, GR, GP)
                        assert w < mp.mpf(10) ** -15, (dn, n, fam, w)
                out[f'{dn}_{n}_{fam}_a'] = a
                for key, v in acc.items():
                    out[f'{dn}_{n}_{fam}_{key}'] = np.asarray(v, np.float64)
            print(dn, n, 'done', flush=True)
    path = os.path.join(HERE, 'polar.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
