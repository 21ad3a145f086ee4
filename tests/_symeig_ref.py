"""Reference model of `sym.sym_eigvals` / `sym.sym_eigh` in numpy: the sort and the sign rule, the gap weights, and the
two gradients in a precision above the working one, with the per-record conditioning the bounds are written in.

High precision: numpy's float64 `eigh` for float32 records, `_symfun_ref.jacobi_eigh` in longdouble for float64 ones.
The model's eigenvectors are aligned to the RETURNED ones by the sign of the inner products (a sign decided by a tie
is unstable; the model must not depend on it).  The gradients follow the formula of the docstring of `sym_eigh`
WITHOUT the gap rule:

    values    S = V diag(gl) V^T
    vectors   S = V W V^T,  W_kl = (B_kl - B_lk) / (2 (l_l - l_k)),  B = V^T gV,  W_kk = 0

Per record, gap = min_k |l_(k+1) - l_k| (ascending) and kappa = |A|_2 / gap.  The bounds, Frobenius norm of the full
symmetric matrix S per record (S is what the formulas bound: |W|_F <= |gV|_F / gap and |diag gl|_F = |gl|_2; the
eigenvectors of a matrix known to n eps |A|_2 move by n eps kappa):

    values    |S - S_model|_F <= C n eps (1 + kappa) |gl|_2
    vectors   |S - S_model|_F <= C n eps (1 + kappa) |gV|_F / gap

A record is judged only if gap >= 64 n eps |A|_2, four times the gap rule.  On the cells 'normal' and 'wilk' of
`_eig_ref.batch` no record may be excluded (the tests assert it)."""
import functools
import numpy as np
import _eig_ref as E
import _symfun_ref as R

C = E.C
NP = R.NP
ORDERS = ('ascending', 'descending', 'abs')
GRAD_CELLS = ('normal', 'wilk')
GAP_RULE = 16.0          # |l_k - l_l| <= GAP_RULE n eps max|l|: the pair's weight is 0
JUDGED = 64.0            # records with gap >= JUDGED n eps |A|_2 are judged


def eps_of(dn):
    return R.eps_of(dn)


# ------------------------------------------------------------------------------------------------ sort, signs, weights
def sort_index(lam, order):
    """the permutation into `order`: by the key, ties by the sign (of the key; of the value for 'abs'): -0.0 before
    +0.0 ascending, after it descending; for 'abs' ties of |l| by the value ascending"""
    if order == 'abs':
        key, tie = np.abs(lam), np.copysign(1.0, lam)
    else:
        key = -lam if order == 'descending' else lam
        tie = np.copysign(1.0, key)
    first = np.argsort(tie, -1, kind='stable')
    second = np.argsort(np.take_along_axis(key, first, -1), -1, kind='stable')
    return np.take_along_axis(first, second, -1)


def key_of(lam, order):
    return np.abs(lam) if order == 'abs' else (-lam if order == 'descending' else lam)


def is_sorted(lam, order):
    """exactly monotone in the key, ties of |l| by the value for 'abs'"""
    k = key_of(lam, order)
    ok = (k[..., 1:] >= k[..., :-1]).all(-1)
    if order == 'abs':
        tie = k[..., 1:] == k[..., :-1]
        ok &= (~tie | (lam[..., 1:] >= lam[..., :-1])).all(-1)
    return ok


def fix_signs(v):
    """the component of largest magnitude of every column positive, the first such component among exact ties"""
    top = np.argmax(np.abs(v), -2)                                  # numpy: the first maximum
    s = np.take_along_axis(v, top[..., None, :], -2)
    return v * np.where(s < 0, -1.0, 1.0).astype(v.dtype)


def signs_ok(v):
    top = np.argmax(np.abs(v), -2)
    return (np.take_along_axis(v, top[..., None, :], -2) > 0).all((-1, -2))


def gap_weights(lam):
    """1 / (l_l - l_k) at [k, l] in the dtype of lam, 0 on the diagonal and where the gap rule says"""
    n = lam.shape[-1]
    d = lam[..., None, :] - lam[..., :, None]
    tol = (lam.dtype.type(GAP_RULE * n) * np.finfo(lam.dtype).eps * np.abs(lam).max(-1))[..., None, None]
    close = np.abs(d) <= tol
    with np.errstate(divide='ignore', over='ignore'):
        return np.where(close, lam.dtype.type(0), lam.dtype.type(1) / np.where(close, lam.dtype.type(1), d)), close


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def grad_batch(dn, n):
    """the records of the cells 'normal' and 'wilk' of `_eig_ref.batch(dn, n)` (plain and shuffled copies): full,
    compact, {cell: slice}"""
    a, cells = E.batch(dn, n)
    idx = np.concatenate([cells[c] for c in GRAD_CELLS])
    full = np.ascontiguousarray(a[idx])
    at, sl = 0, {}
    for c in GRAD_CELLS:
        sl[c] = slice(at, at + len(cells[c]))
        at += len(cells[c])
    comp = R.pack(full)
    for x in (full, comp):
        x.setflags(write=False)
    return full, comp, sl


@functools.lru_cache(maxsize=None)
def cotangents(dn, n, nb, seed=23):
    rng = np.random.default_rng(seed + n)
    gl = rng.standard_normal((nb, n)).astype(NP[dn])
    gv = rng.standard_normal((nb, n, n)).astype(NP[dn])
    for x in (gl, gv):
        x.setflags(write=False)
    return gl, gv


@functools.lru_cache(maxsize=None)
def _eigh_hp(dn, n):
    """high-precision ascending decomposition of grad_batch(dn, n), once"""
    return R.eigh_hp(dn, grad_batch(dn, n)[0])


# ------------------------------------------------------------------------------------------------ the model
def model(dn, full, order, vecs, gl=None, gv=None, hp=None):
    """high-precision gradients of the records `full` for the returned eigenvectors `vecs` (used for the signs only).
    Returns {'gl': S of the values' cotangent, 'gv': S of the vectors' cotangent, 'gap', 'kappa', 'norm'}; S full
    symmetric matrices in high precision"""
    lam, v = hp if hp is not None else R.eigh_hp(dn, np.asarray(full))
    H = lam.dtype.type
    norm = np.abs(lam).max(-1).astype(np.float64)
    gap = np.diff(lam, axis=-1).min(-1).astype(np.float64) if lam.shape[-1] > 1 else np.full(len(lam), np.inf)
    idx = sort_index(lam, order)
    lam = np.take_along_axis(lam, idx, -1)
    v = np.take_along_axis(v, idx[:, None, :], -1)
    dots = np.einsum('bik,bik->bk', v, np.asarray(vecs).astype(lam.dtype))
    v = v * np.where(dots < 0, H(-1), H(1))[:, None, :]
    out = {'gap': gap, 'norm': norm}
    with np.errstate(divide='ignore', invalid='ignore'):
        out['kappa'] = np.where(gap > 0, norm / gap, np.inf)
    if gl is not None:
        out['gl'] = np.einsum('bik,bk,bjk->bij', v, np.asarray(gl).astype(lam.dtype), v)
    if gv is not None:
        b = np.einsum('bik,bil->bkl', v, np.asarray(gv).astype(lam.dtype))
        d = lam[:, None, :] - lam[:, :, None]
        eye = np.eye(lam.shape[-1], dtype=bool)
        with np.errstate(divide='ignore', invalid='ignore'):
            w = np.where(eye, H(0), H(0.5) * (b - b.swapaxes(-1, -2)) / np.where(eye, H(1), d))
        out['gv'] = np.einsum('bik,bkl,bjl->bij', v, w, v)
    return out


def judged(dn, n, mod):
    return mod['gap'] >= JUDGED * n * eps_of(dn) * mod['norm']


def _fro(x):
    return np.sqrt((np.asarray(x, np.float64) ** 2).sum(tuple(range(1, np.ndim(x)))))


def grad_ratio(dn, n, mod, got, gl=None, gv=None):
    """per record |S_got - S_model|_F / bound with C = 1 (compare with C); `got` the compact gradient (S_ii, 2 S_ij);
    with both cotangents the bound is the sum of the two"""
    want = 0
    bound = 0
    cond = n * eps_of(dn) * (1 + mod['kappa'])
    if gl is not None:
        want = want + mod['gl']
        bound = bound + cond * _fro(gl)
    if gv is not None:
        want = want + mod['gv']
        bound = bound + cond * _fro(gv) / mod['gap']
    s = R.unpack(np.asarray(got), n, off=0.5).astype(want.dtype)
    err = _fro((s - want).astype(np.float64))
    err = np.where(np.isfinite(np.asarray(got)).all(-1), err, np.inf)
    return E._ratio(err, bound)
