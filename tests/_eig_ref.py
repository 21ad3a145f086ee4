"""Inputs and per-record judges of eig_sym on hard spectra and across the exponent range (shared by
test_eig_sym_accuracy_host.py, which holds the ORACLE to them, test_gpu_eig_sym_accuracy.py, which holds the
kernels to them, and scripts/eig_sym_accuracy_scan.py, which writes profiles/eig_sym_accuracy.md).

Why per record: `conftest.relerr` divides by the largest entry of the whole batch and `check_eigenpairs` uses
one scale for all records, so a record that is small next to its neighbours can be entirely wrong and pass.
Here every record is scored against ITS OWN 2-norm:

    values          |sort(got) - truth|_max            / (n eps |A|_2)     (less one subnormal step of the dtype)
    residual        |A U - U diag(got)|_max            / (n eps |A|_2)
    orthogonality   |U^T U - I|_max                    / (n eps)

truth = numpy.linalg.eigvalsh in float64 of the record AS ROUNDED to the dtype and scaled by the exact power of
two that brings its largest entry into [1, 2) (so that LAPACK itself never leaves its range; its own error, a
few n 2^-53, is inside C for float64 and invisible for float32).  Results are scaled by the same power of two
before they are compared, which is exact.  Residual and orthogonality are evaluated in float64 for float32
results and in numpy.longdouble for float64 results (HIGH_EPS below says what that is on this machine).
A non-finite result for finite input scores inf.

A CELL is (family, 64 records); a ratio of a cell is the worst of its records, in the plain batch and in the
copy that is shuffled record by record (every range decision of the kernels is a wavefront vote: the shuffled
copy mixes scales and families inside every wavefront).

The bar C.  It is the next power of two at or above 4 x the worst ratio of the oracle over the cells in which
the reference-order arithmetic is sound (everything but REFERENCE_EXCEEDS), shared by both dtypes:
profiles/eig_sym_accuracy.md has the scan (worst sound ratio 3.97 -> C = 16).  The reference-order arithmetic
may exceed C only in the cells of REFERENCE_EXCEEDS, and must exceed it there (the list cannot rot);
arithmetic='fast' has no exclusions."""
import functools
import numpy as np

NP = {'f32': np.float32, 'f64': np.float64}
ORDERS = (2, 3, 4, 5, 6, 8, 9, 12, 13, 16)
PER_CELL = 64
C = 16.0
FAMILIES = ('normal', 'graded', 'gradedrows', 'repeated', 'cluster', 'rank1', 'wilk')
SWEEP_FAMILIES = ('normal', 'graded')
SWEEP = {'f32': (-100, -80, -70, -66, -63, -60, -40, 0, 40, 56, 60, 63, 64, 100, 120),
         'f64': (-960, -600, -520, -512, -500, -300, 0, 300, 500, 508, 512, 600, 1000)}
METRICS = ('values', 'residual', 'orthogonality')
# what the high-precision evaluation of a float64 result adds: nothing where longdouble is the x87 format
HIGH_EPS = float(np.finfo(np.longdouble).eps)
HIGH_OK = HIGH_EPS < 2.0 ** -60

# Cells (dtype, n, family, metric) in which the REFERENCE-ORDER arithmetic exceeds C.  This is upstream's
# arithmetic, restated: `tol = 1e-32` asks float32 for |e| < 1e-16 |d|, which repeated and clustered eigenvalues
# never reach, so those stages run all max_iter = 1024 sweeps and drift; and its rotations and reflectors
# normalise by an unscaled sum of squares, which underflows for the tiny pairs that such spectra (and rank-one
# matrices) leave inside a unit-scale matrix, so the eigenvectors lose orthogonality.  No scale-sweep cell is
# here.  arithmetic='fast' is the mode to use on such spectra in float32.
# (filled from scripts/eig_sym_accuracy_scan.py; test_eig_sym_accuracy_host.py asserts both directions)
REFERENCE_EXCEEDS = frozenset({                    # the oracle's ratio
    ('f32', 3, 'rank1', 'orthogonality'),          # 16.5
    ('f32', 6, 'repeated', 'orthogonality'),       # 82.5
    ('f32', 6, 'cluster', 'orthogonality'),        # 16.3
    ('f32', 8, 'repeated', 'residual'),            # 19.3
    ('f32', 8, 'repeated', 'orthogonality'),       # 92
    ('f32', 8, 'cluster', 'orthogonality'),        # 25.6
    ('f32', 9, 'repeated', 'orthogonality'),       # 44.7
    ('f32', 9, 'cluster', 'orthogonality'),        # 71
    ('f32', 12, 'repeated', 'orthogonality'),      # 67.3
    ('f32', 12, 'cluster', 'orthogonality'),       # 36.6
    ('f32', 13, 'repeated', 'orthogonality'),      # 74.5
    ('f32', 13, 'cluster', 'orthogonality'),       # 51.4
    ('f32', 16, 'repeated', 'residual'),           # 22.9
    ('f32', 16, 'repeated', 'orthogonality'),      # 61.1
    ('f32', 16, 'cluster', 'orthogonality'),       # 67.8
    ('f32', 16, 'wilk', 'values'),                 # 39.5
    ('f32', 16, 'wilk', 'residual'),               # 19.4
    ('f32', 16, 'wilk', 'orthogonality'),          # 61.6
})


def eps_of(dn):
    return float(np.finfo(NP[dn]).eps)


# ------------------------------------------------------------------------------------------------ generators
def _orth(rng, nb, n):
    q, r = np.linalg.qr(rng.standard_normal((nb, n, n)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def _from_spectrum(rng, lam):
    q = _orth(rng, *lam.shape)
    a = np.einsum('bij,bj,bkj->bik', q, lam, q)
    return (a + a.swapaxes(-1, -2)) / 2


def family(name, rng, nb, n):
    """nb float64 symmetric records of one family at unit scale"""
    if name == 'normal':
        a = rng.standard_normal((nb, n, n))
        return (a + a.swapaxes(-1, -2)) / 2
    if name == 'graded':                          # eigenvalues 1 ... 1e-6, log-spaced, random signs
        lam = 10.0 ** (-6.0 * np.arange(n) / max(n - 1, 1)) * rng.choice([-1.0, 1.0], (nb, n))
        return _from_spectrum(rng, lam)
    if name == 'gradedrows':                      # D A D, D = diag(1 ... 1e-3)
        a = rng.standard_normal((nb, n, n))
        d = 10.0 ** (-3.0 * np.arange(n) / max(n - 1, 1))
        return (a + a.swapaxes(-1, -2)) / 2 * d[:, None] * d[None, :]
    if name == 'repeated':                        # -0.5 on half, 1 on the rest
        lam = np.where(np.arange(n) < n // 2, -0.5, 1.0) * np.ones((nb, 1))
        return _from_spectrum(rng, lam)
    if name == 'cluster':                         # 1 + 1e-6 N(0, 1), one at -2
        lam = 1.0 + 1e-6 * rng.standard_normal((nb, n))
        lam[:, 0] = -2.0
        return _from_spectrum(rng, lam)
    if name == 'rank1':
        v = rng.standard_normal((nb, n))
        return v[:, :, None] * v[:, None, :]
    if name == 'wilk':                            # Wilkinson's W+ times a random factor in [0.5, 2]
        w = np.diag(np.abs(np.arange(n) - (n - 1) / 2.0)) + np.eye(n, k=1) + np.eye(n, k=-1)
        return w[None] * rng.uniform(0.5, 2.0, (nb, 1, 1))
    raise ValueError(name)


def specials(rng, n):
    """the exact-zero structures of the existing tests: 8 zero, 16 diagonal, 16 block-diagonal records, 8 with
    a leading 2 x 2 block of equal diagonal (delta = 0: the closed-form last stage's t = +-1), and 5 more unit
    ones so that the batch length is no multiple of 64.  Returns {cell: records}"""
    out = {'zero': np.zeros((8, n, n)), 'diagonal': np.eye(n) * rng.standard_normal((16, 1, n))}
    b = family('normal', rng, 16, n)
    b[:, 0, 1:] = 0.0
    b[:, 1:, 0] = 0.0
    out['blockdiag'] = b
    d = np.eye(n) * rng.standard_normal((8, 1, n))
    d[:, 0, 0] = d[:, 1, 1] = 2.0
    d[:, 0, 1] = d[:, 1, 0] = 5.0
    out['delta0'] = d
    out['tail'] = family('normal', rng, 5, n)
    return out


@functools.lru_cache(maxsize=None)
def batch(dn, n):
    """(a, cells): `a` the records of every cell back to back and then the same records shuffled one by
    one; cells = {name: indices into a (both copies)}; all frozen.  Seeded per (dtype, n)."""
    dtype = NP[dn]
    rng = np.random.default_rng(7100 + 100 * (dn == 'f64') + n)
    parts = {f: family(f, rng, PER_CELL, n) for f in FAMILIES}
    for f in SWEEP_FAMILIES:
        for k in SWEEP[dn]:
            parts[f'{f}*2^{k}'] = np.ldexp(family(f, rng, PER_CELL, n), k)
    tiny = float(np.finfo(dtype).tiny)
    parts['subnormal*4'] = family('normal', rng, PER_CELL, n) * (4 * tiny)      # a fifth of the entries subnormal
    # nearly every entry subnormal; no smaller: n eps |A|_2 must stay at or above one subnormal step (2^-149 / 2^-1074),
    # as in the scale sweep, or the bars ask for less than the dtype can represent
    parts['subnormal/2'] = family('normal', rng, PER_CELL, n) * (tiny / 2)
    parts.update(specials(rng, n))
    with np.errstate(under='ignore'):
        a = np.concatenate(list(parts.values())).astype(dtype)
    a = (np.tril(a) + np.tril(a, -1).swapaxes(-1, -2)).astype(dtype)             # symmetric after rounding
    nb = len(a)
    assert nb % 64 != 0
    perm = rng.permutation(nb)
    cells, at = {}, 0
    where = np.empty(nb, np.int64)
    where[perm] = np.arange(nb)                   # record i of the plain copy is record nb + where[i] of the batch
    for name, p in parts.items():
        idx = np.arange(at, at + len(p))
        cells[name] = np.concatenate([idx, nb + where[idx]])
        cells[name].setflags(write=False)
        at += len(p)
    a = np.concatenate([a, a[perm]])
    a.setflags(write=False)
    return a, cells


def cell_family(cell):
    return cell.split('*')[0] if '*2^' in cell else cell


def is_sweep(cell):
    return '*2^' in cell


# ------------------------------------------------------------------------------------------------ judges
def scale_exponent(a):
    """per record, e with max|a_ij| in [2^e, 2^(e+1)); 0 for a zero record"""
    m = np.abs(a).max((-1, -2)).astype(np.float64)
    return np.where(m > 0, np.frexp(m)[1] - 1, 0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def truth(dn, n):
    """(e, a_s, lam, norm2): the scaling exponents, the records scaled into [1, 2) in float64, their eigenvalues
    by numpy.linalg.eigvalsh (ascending) and their 2-norms"""
    a = batch(dn, n)[0]
    e = scale_exponent(a)
    a_s = np.ldexp(a.astype(np.float64), -e[:, None, None])
    lam = np.linalg.eigvalsh(a_s)
    return e, a_s, lam, np.abs(lam).max(-1)


def _ratio(err, den):
    """err / den per record; 0 / 0 = 0, x / 0 = inf, anything non-finite = inf"""
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err <= 0, 0.0, np.where(den > 0, err / den, np.inf))


def judge_values(dn, n, vals, a=None, tr=None):
    """per-record ratio of eigenvalues `vals` (any order).  a / tr: other records than batch(dn, n) and
    their truth (`truth_of`)"""
    e, _, lam, nrm = tr if tr is not None else truth(dn, n)
    with np.errstate(invalid='ignore', over='ignore'):
        g = np.ldexp(np.sort(vals.astype(np.float64), -1), -e[:, None])
        step = np.ldexp(float(np.finfo(NP[dn]).smallest_subnormal), -e)
        err = np.abs(g - lam).max(-1) - step
    err = np.where(np.isfinite(vals).all(-1), err, np.inf)
    return _ratio(err, n * eps_of(dn) * nrm)


def judge_vectors(dn, n, vals, vecs, tr=None):
    """per-record (residual ratio, orthogonality ratio) of eigenpairs"""
    e, a_s, _, nrm = tr if tr is not None else truth(dn, n)
    hi = np.float64 if dn == 'f32' else np.longdouble
    extra = 0.0 if (dn == 'f32' or HIGH_OK) else 1.0         # n eps more where longdouble is only float64
    with np.errstate(invalid='ignore', over='ignore'):
        g = np.ldexp(vals.astype(np.float64), -e[:, None]).astype(hi)
        u = vecs.astype(hi)
        res = np.abs(np.einsum('bij,bjk->bik', a_s.astype(hi), u) - u * g[:, None, :]).max((-1, -2)).astype(np.float64)
        orth = np.abs(np.einsum('bji,bjk->bik', u, u) - np.eye(n, dtype=hi)).max((-1, -2)).astype(np.float64)
    fin = np.isfinite(vals).all(-1) & np.isfinite(vecs).all((-1, -2))
    res, orth = np.where(fin, res, np.inf), np.where(fin, orth, np.inf)
    den = n * eps_of(dn)
    return np.maximum(_ratio(res, den * nrm) - extra, 0.0), np.maximum(_ratio(orth, den) - extra, 0.0)


def truth_of(a):
    """`truth` for records that are not a batch of this module (the amended range tests)"""
    e = scale_exponent(a)
    a_s = np.ldexp(a.astype(np.float64), -e[:, None, None])
    lam = np.linalg.eigvalsh(a_s)
    return e, a_s, lam, np.abs(lam).max(-1)


def judge(dn, n, vals, vals_u, vecs, tr=None):
    """{metric: per-record ratios}; `values` is the worse of the values-only call and the call with vectors"""
    res, orth = judge_vectors(dn, n, vals_u, vecs, tr)
    v = np.maximum(judge_values(dn, n, vals, tr=tr), judge_values(dn, n, vals_u, tr=tr))
    return {'values': v, 'residual': res, 'orthogonality': orth}


def per_cell(dn, n, ratios):
    """{(cell, metric): worst ratio of the cell}"""
    cells = batch(dn, n)[1]
    return {(c, m): float(ratios[m][idx].max()) for c, idx in cells.items() for m in METRICS}


def exceeding(dn, n, worst, bar=C):
    """the cells of `worst` (per_cell) above the bar, as REFERENCE_EXCEEDS spells them"""
    return {(dn, n, c, m) for (c, m), r in worst.items() if not r <= bar}


def listed(dn, n):
    return {x for x in REFERENCE_EXCEEDS if x[0] == dn and x[1] == n}


def same_value_set(dn, n, vals, vals_u, tr=None):
    """per-record |sort(vals) - sort(vals_u)|_max / (n eps |A|_2): the two kernels of one arithmetic mode return
    the same SET of eigenvalues (bar: 2 C)"""
    e, _, _, nrm = tr if tr is not None else truth(dn, n)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.abs(np.ldexp(np.sort(vals.astype(np.float64), -1), -e[:, None])
                   - np.ldexp(np.sort(vals_u.astype(np.float64), -1), -e[:, None])).max(-1)
        d = d - 2 * np.ldexp(float(np.finfo(NP[dn]).smallest_subnormal), -e)
    return _ratio(d, n * eps_of(dn) * nrm)


@functools.lru_cache(maxsize=None)
def oracle_results(oracle, dn, n):
    """the oracle on batch(dn, n), once: (values, values of the call with vectors, vectors), frozen"""
    a = batch(dn, n)[0]
    vals = oracle.eig_sym(a)
    vals_u, vecs = oracle.eig_sym(a, True)
    for x in (vals, vals_u, vecs):
        x.setflags(write=False)
    return vals, vals_u, vecs


def assert_records_within(dn, n, a, vals, vals_u, vecs, bar=C):
    """every record of `a` (any finite symmetric records of sound families) within the bar, on all three metrics"""
    r = judge(dn, n, vals, vals_u, vecs, truth_of(a))
    for m, x in r.items():
        i = int(np.argmax(x))
        assert x[i] <= bar, (m, i, float(x[i]), float(np.abs(a[i]).max()))
