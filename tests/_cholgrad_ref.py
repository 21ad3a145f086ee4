"""Reference model of the gradients of the Cholesky factor of `sym` (the backward pass of sym_chol and of the four ops
of sym_chol_apply, with respect to the matrix -- or, with `factored`, to the factor -- and to the vector): cotangents, a
high-precision model and per-record first-order error bounds.  numpy only; the inputs, the plain routines and the
forward quantities are those of tests/_symchol_ref.py.

The formulas (L the factor, G the compact cotangent of L, one value per stored entry; g the cotangent of an applied
vector; Sym(X) = the symmetric matrix whose lower triangle, diagonal included, is that of X, which is Phi(X) + Phi(X)^T
with Phi = the lower triangle with a halved diagonal):
    factor     S = L^-T Sym(L^T G) L^-1 / 2
    'L'        gv = L^T g,    G = tril(g v^T)          'LT'       gv = L g,     G = tril(v g^T)
    'Linv'     gv = L^-T g,   G = -tril(gv y^T), y = L^-1 v
    'LTinv'    gv = L^-1 g,   G = -tril(y gv^T), y = L^-T v
and S from G by the first line unless `factored`, where G itself is the gradient.  The compact S is (S_ii, 2 S_ij).

The bounds (per record, elementwise, first order; gamma = (n + 2) eps).  The computed factor carries
    |dL| <= gamma |L| (|L^-1| P |L^-T|),  P = |L||L^T|                  (tests/_symchol_ref.py; zero with `factored`)
and whatever is obtained by substitution with it carries
    |d(L^-1)| <= |L^-1| |dL| |L^-1| + gamma |L^-1| |L| |L^-1|
(the second term is the backward error of a substitution, |dL| <= gamma |L| per right-hand side).  Both are carried
through every formula above by the product rule -- an intermediate (y, gv, G) hands its own bound on -- and every formula
adds gamma times itself evaluated with absolute values for the rounding of its own sums.  These are rigorous first-order
bounds, valid under the condition `judged` of tests/_symchol_ref.py; the bar is a ratio <= 1 in every cell.
"""
import functools
import numpy as np
import _symchol_ref as C
import _symfun_ref as R

NP, HP = R.NP, R.HP
OPS = ('factor',) + C.APPLY
_mm, _mv = C._mm, C._mv


def _t(x):
    return x.swapaxes(-1, -2)


def _outer(a, b):
    return a[:, :, None] * b[:, None, :]


def sym_lower(x):
    """Sym(X): the symmetric matrix with the lower triangle (diagonal included) of X"""
    return np.tril(x) + _t(np.tril(x, -1))


def lower_of(comp, n):
    """full lower-triangular matrices from compact factors (or compact cotangents of a factor)"""
    return np.tril(R.unpack(np.asarray(comp), n))


def pack_lower(full):
    """compact storage of the lower triangle of `full`"""
    return R.pack(_t(full))


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def cotangents(dn, n, nb=C.NB):
    """(cotangents of the factor (nb, K), cotangents of an applied vector (nb, n)) of the dtype, read-only"""
    rng = np.random.default_rng(6000 + 10 * n + (dn == 'f64'))
    G = rng.standard_normal((nb, n * (n + 1) // 2)).astype(NP[dn])
    g = rng.standard_normal((nb, n)).astype(NP[dn])
    G.setflags(write=False)
    g.setflags(write=False)
    return G, g


@functools.lru_cache(maxsize=None)
def factor_input(dn, n):
    """the compact factors of C.batch(dn, n) that the `factored` calls are given: the plain numpy Cholesky in the working
    precision (an input like any other: the model takes it as exact)"""
    comp = C.batch(dn, n)[0]
    f = pack_lower(C.chol_any(R.unpack(np.asarray(comp, NP[dn]), n))).astype(NP[dn])
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------ the formulas
def _inverse_lower(l):
    eye = np.broadcast_to(np.eye(l.shape[-1], dtype=l.dtype), l.shape)
    return C.solve_lower(l, eye.copy())


def _pullback(l, linv, G):
    """S (full, symmetric) from the cotangent G (full lower) of the factor"""
    return _mm(_t(linv), _mm(sym_lower(_mm(_t(l), G)), linv)) / 2


def _pullback_bound(gm, l, linv, dl, dlinv, G, dG):
    al, alinv, aG = np.abs(l), np.abs(linv), np.abs(G)
    m = np.abs(sym_lower(_mm(_t(l), G)))
    dm = sym_lower(_mm(_t(dl), aG) + _mm(_t(al), dG))
    mabs = sym_lower(_mm(_t(al), aG))
    first = _mm(_t(dlinv), _mm(m, alinv)) + _mm(_t(alinv), _mm(dm, alinv)) + _mm(_t(alinv), _mm(m, dlinv))
    return first / 2 + gm * _mm(_t(alinv), _mm(mabs, alinv)) / 2


def _apply_parts(op, l, linv, v, g):
    """(gv, G full lower) of an apply op, in the precision of the arguments"""
    if op == 'L':
        return _mv(_t(l), g), np.tril(_outer(g, v))
    if op == 'LT':
        return _mv(l, g), np.tril(_outer(v, g))
    if op == 'Linv':
        y, gv = _mv(linv, v), _mv(_t(linv), g)
        return gv, -np.tril(_outer(gv, y))
    y, gv = _mv(_t(linv), v), _mv(linv, g)
    return gv, -np.tril(_outer(y, gv))


def _apply_bounds(gm, op, l, linv, dl, dlinv, v, g):
    """(bound of gv, bound of G) of an apply op"""
    al, alinv, av, ag = np.abs(l), np.abs(linv), np.abs(v), np.abs(g)
    if op == 'L':
        return _mv(_t(dl), ag) + gm * _mv(_t(al), ag), gm * np.tril(_outer(ag, av))
    if op == 'LT':
        return _mv(dl, ag) + gm * _mv(al, ag), gm * np.tril(_outer(av, ag))
    if op == 'Linv':
        y, gv = np.abs(_mv(linv, v)), np.abs(_mv(_t(linv), g))
        dy = _mv(dlinv, av) + gm * _mv(alinv, av)
        dgv = _mv(_t(dlinv), ag) + gm * _mv(_t(alinv), ag)
        return dgv, np.tril(_outer(dgv, y) + _outer(gv, dy) + gm * _outer(gv, y))
    y, gv = np.abs(_mv(_t(linv), v)), np.abs(_mv(linv, g))
    dy = _mv(_t(dlinv), av) + gm * _mv(_t(alinv), av)
    dgv = _mv(dlinv, ag) + gm * _mv(alinv, ag)
    return dgv, np.tril(_outer(dy, gv) + _outer(y, dgv) + gm * _outer(y, gv))


def model(dn, n, mat, factored):
    """what every gradient needs of the matrix operand, in high precision: L, L^-1 and the bounds of both"""
    hp = HP[dn]
    gm = C.gamma(dn, n)
    if factored:
        l = lower_of(np.asarray(mat).astype(hp), n)
        dl = np.zeros_like(l)
    else:
        l = C.chol_any(R.unpack(np.asarray(mat).astype(hp), n))
    linv = _inverse_lower(l)
    al, alinv = np.abs(l), np.abs(linv)
    if not factored:
        dl = gm * _mm(al, _mm(alinv, _mm(_mm(al, _t(al)), _t(alinv))))
    dlinv = _mm(alinv, _mm(dl, alinv)) + gm * _mm(alinv, _mm(al, alinv))
    return dict(n=n, gm=gm, l=l, linv=linv, dl=dl, dlinv=dlinv, factored=bool(factored))


@functools.lru_cache(maxsize=None)
def truth(dn, n, factored):
    """model of C.batch(dn, n) (or, factored, of factor_input(dn, n)); computed once"""
    return model(dn, n, factor_input(dn, n) if factored else C.batch(dn, n)[0], factored)


def want(dn, m, op, vec, cot):
    """(gradient with respect to the matrix operand, its bound, gradient with respect to the vector, its bound); the
    first pair is full symmetric S, or with `factored` the full lower G; the second is None for op 'factor'"""
    hp = HP[dn]
    n, gm, l, linv, dl, dlinv = m['n'], m['gm'], m['l'], m['linv'], m['dl'], m['dlinv']
    if op == 'factor':
        G = lower_of(np.asarray(cot).astype(hp), n)
        gv = bv = None
        dG = np.zeros_like(G)
    else:
        v, g = np.asarray(vec).astype(hp), np.asarray(cot).astype(hp)
        gv, G = _apply_parts(op, l, linv, v, g)
        bv, dG = _apply_bounds(gm, op, l, linv, dl, dlinv, v, g)
    if m['factored'] and op != 'factor':
        return G, dG, gv, bv
    return _pullback(l, linv, G), _pullback_bound(gm, l, linv, dl, dlinv, G, dG), gv, bv


def ratio(dn, m, op, got, vec, cot):
    """per record: the largest error of the packed gradient `got` ([K], or [K | n] for an apply op) over its bound"""
    hp = HP[dn]
    n = m['n']
    K = n * (n + 1) // 2
    got = np.asarray(got).astype(hp)
    S, bS, gv, bv = want(dn, m, op, vec, cot)
    if m['factored'] and op != 'factor':
        S_got = lower_of(got[:, :K], n)
    else:
        S_got = R.unpack(got[:, :K], n, off=0.5)
    r = C._ratio(np.abs(S_got - S), bS)
    if op != 'factor':
        r = np.maximum(r, C._ratio(np.abs(got[:, K:] - gv), bv))
    return r


# ------------------------------------------------------------------------------------------------ plain routine
def plain(dn, n, op, mat, vec, cot, factored):
    """the packed gradient from the plain routines of tests/_symchol_ref.py in the WORKING precision (substitutions
    and products from the definition, no fused operations): what the bounds are validated with"""
    T = NP[dn]
    if factored:
        l = lower_of(np.asarray(mat, T), n)
    else:
        l = C.chol_any(R.unpack(np.asarray(mat, T), n))
    lt = _t(l)
    if op == 'factor':
        G, gv = lower_of(np.asarray(cot, T), n), None
    else:
        v, g = np.asarray(vec, T), np.asarray(cot, T)
        if op == 'L':
            gv, G = _mv(lt, g), np.tril(_outer(g, v))
        elif op == 'LT':
            gv, G = _mv(l, g), np.tril(_outer(v, g))
        elif op == 'Linv':
            y, gv = C.solve_lower(l, v), C.solve_upper(lt, g)
            G = -np.tril(_outer(gv, y))
        else:
            y, gv = C.solve_upper(lt, v), C.solve_lower(l, g)
            G = -np.tril(_outer(y, gv))
    if factored and op != 'factor':
        head = pack_lower(G)
    else:
        x = C.solve_upper(lt, sym_lower(_mm(lt, G)))                 # L^-T M
        head = R.pack(C.solve_upper(lt, _t(x)) * T(0.5), off=2.0)    # L^-T (M L^-1)
    return (head if gv is None else np.concatenate([head, gv], -1)).astype(T)
