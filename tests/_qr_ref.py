"""Inputs, truths and per-record judges of the QR building blocks at orders 1..8: givens, givens_apply,
householder, householder_apply, hessenberg, hessenberg_sym, qr_hessenberg, rq_hessenberg (shared by
test_qr_family_host.py, which holds the ORACLE to every bound below, and test_gpu_qr_family.py, which holds the
kernels to them and to the oracle, bit for bit).  numpy only, written from the definitions.

Why per record: `conftest.relerr` divides the largest error of the whole batch by the largest entry of the whole
batch, so a record that is small next to its neighbours can be entirely wrong and pass.  Here every record is
scored against ITS OWN Frobenius norm, in numpy.longdouble, and every score is a RATIO: error / bound-without-C.
A record passes when its ratio is <= C = 16, the project's constant (`check_eigenpairs`, `_eig_ref.C`).  A zero
bound demands a zero error (ratio 0, else inf); a non-finite result for finite input scores inf; the exact
demands (structural zeros, u = 0 for x = 0, bit-for-bit identities) score 0 or inf.

    householder        |(I - 2 u u^T) x - alpha e_b| / (n eps |x|),   ||alpha| - |x|| / (n eps |x|),
                       ||u| - 1| / eps,   u = 0 and alpha = 0 exactly for x = 0,   upstream's sign rule
                       (alpha = -sign(x_b) |x|, sign(0) = -1: alpha >= 0 for x_b <= 0)
    givens             |c^2 + s^2 - 1| / (2 eps),   |s x + c y| / (2 eps r),   |c x - s y - r| / (2 eps r),
                       (0, 0) -> (1, 0), (x, 0) -> (sign x, 0), (0, y) -> (0, -sign y) exactly
    hessenberg         |Q H Q^T - A| / (n eps |A|) with Q = P_0 P_1 ... built from the RETURNED reflectors (a
                       reflector that is not of unit length shows here), exact zeros below the subdiagonal, the
                       same H with and without compute_u, zero and diagonal records back exactly
    hessenberg_sym     the same against the mirrored triangle that is read, GENERAL records and both `upper`
                       (reading the wrong triangle shows); fill=True: exact zeros outside the three diagonals
                       and an exactly symmetric result; fill=False: the other triangle is the input's
    qr_hessenberg      |Q R - H| / (n eps |H|),   |Q^T Q - I| / (n eps),   |tril(R, -1)| / (n eps |H|)
                       (upstream rotates R's subdiagonal and does not zero it: no exact zeros are asked there)
    rq_hessenberg      with the same backend's q, r:  |RQ - r q| / (n eps |H|),   |q RQ q^T - H| / (2 n eps |H|),
                       with u:  |u' - u q| / (n eps |u|)
    householder_apply  against the dense longdouble product / (n eps |A|); u = 0 leaves A bit for bit
    givens_apply       against the dense longdouble product / (n eps |A|); (c, s) = (1, 0) leaves A bit for bit

The batch: NB = 2 * 512 + 176 records per (dtype, order) -- two full tiles of the largest tile of the record
kernel and a ragged tail, no multiple of 64 -- the families below back to back and then shuffled record by
record (every range decision of the kernels is a wavefront vote: the shuffle mixes scales and families inside
every wavefront).  Frozen and cached.

Two families put tiny columns into a record: `tiny rows` (rows 2.. times 2^-s: what hessenberg, qr_hessenberg and
rq_hessenberg reflect or rotate at step 1 is tiny, the rows it is applied to from the right are O(1)) and `tiny border`
(symmetric, row and column 0 off the diagonal times 2^-s, the trailing block O(1): the first reflector of hessenberg_sym,
in both `upper` settings, and of hessenberg comes from a tiny column and is applied to an O(1) block)."""
import functools
import numpy as np

NP = {'f32': np.float32, 'f64': np.float64}
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
ORDERS = tuple(range(1, 9))
NB = 2 * 512 + 176
C = 16.0
HI = np.longdouble          # the x87 format where these tests run: 64-bit significand, squares of 2^-535 in range
SIDES = ('left', 'right', 'both')
TINY_SHIFTS = {'f32': (40, 62, 66, 70, 73), 'f64': (300, 505, 515, 525, 535)}   # rows 2.. times 2^-s
SCALE = {'f32': 30, 'f64': 200}                  # whole record times 2^+-SCALE
TINY = {'f32': -70, 'f64': -525}                 # vectors and pairs at 2^TINY
GRADE = {'f32': 3.0, 'f64': 6.0}                 # condition 1e3 / 1e6 of the graded families


def eps_of(dn):
    return EPS[dn]


def _frozen(x):
    x.setflags(write=False)
    return x


def _assemble(parts, dtype, rng):
    """parts {family: records} -> (records shuffled one by one, {family: indices})"""
    with np.errstate(under='ignore', over='ignore'):
        a = np.concatenate(list(parts.values())).astype(dtype)
    a = a + dtype(0)                             # every zero is +0 (the bit-for-bit demands of the apply judges)
    assert len(a) == NB and NB % 64 != 0, len(a)
    perm = rng.permutation(NB)
    where = np.empty(NB, np.int64)
    where[perm] = np.arange(NB)                  # record i of the plain order is record where[i] of the batch
    cells, at = {}, 0
    for name, p in parts.items():
        cells[name] = _frozen(np.sort(where[at:at + len(p)]))
        at += len(p)
    return _frozen(a[perm]), cells


# ------------------------------------------------------------------------------------------------ inputs
def tiny_border(a, s):
    """symmetric records whose row and column 0, off the diagonal, are 2^-s of the O(1) trailing block: whichever
    triangle is read, the first reflected column is tiny and the block the reflector is applied to is not (a
    `tiny rows` record read as symmetric has a tiny trailing block: a wrong reflector cannot hurt it)"""
    a = (a + a.swapaxes(-1, -2)) / 2
    a[:, 1:, 0] = np.ldexp(a[:, 1:, 0], -s)
    a[:, 0, 1:] = a[:, 1:, 0]
    return a


@functools.lru_cache(maxsize=None)
def matrices(dn, n):
    """(a, cells): NB general n x n records and {family: indices}"""
    rng = np.random.default_rng(8100 + 100 * (dn == 'f64') + n)
    g = 10.0 ** (-GRADE[dn] * np.arange(n) / max(n - 1, 1))

    def nrm(k):
        return rng.standard_normal((k, n, n))

    def ints(k):
        return rng.integers(-4, 5, (k, n)).astype(np.float64)

    p = {'normal': nrm(64), 'graded rows': nrm(56) * g[:, None], 'graded cols': nrm(56) * g[None, :]}
    z = nrm(56)
    z[:, 2:, 0] = 0.0
    p['zero subcolumn'] = z
    p['hessenberg'] = np.triu(nrm(56), -1)
    p['diagonal'] = np.eye(n) * rng.standard_normal((40, 1, n))
    p['zero'] = np.zeros((16, n, n))
    p['integer rank 1'] = ints(56)[:, :, None] * ints(56)[:, None, :]
    p['integer rank 2'] = ints(56)[:, :, None] * ints(56)[:, None, :] + ints(56)[:, :, None] * ints(56)[:, None, :]
    p['outer'] = rng.standard_normal((192, n, 1)) * rng.standard_normal((192, 1, n))
    p[f'*2^{SCALE[dn]}'] = np.ldexp(nrm(56), SCALE[dn])
    p[f'*2^-{SCALE[dn]}'] = np.ldexp(nrm(56), -SCALE[dn])
    for s in TINY_SHIFTS[dn]:
        t = nrm(64)
        t[:, 2:, :] = np.ldexp(t[:, 2:, :], -s)
        p[f'tiny rows 2^-{s}'] = t
    for s in TINY_SHIFTS[dn]:
        p[f'tiny border 2^-{s}'] = tiny_border(nrm(24), s)
    return _assemble(p, NP[dn], rng)


@functools.lru_cache(maxsize=None)
def hessenbergs(dn, n):
    """triu(., -1) of the same records (qr_hessenberg, rq_hessenberg)"""
    return _frozen(np.triu(matrices(dn, n)[0], -1))


@functools.lru_cache(maxsize=None)
def vectors(dn, n, b):
    """(x, cells): NB vectors of length n for householder with basis b"""
    rng = np.random.default_rng(8300 + 100 * (dn == 'f64') + 10 * n + (b != 0))

    def nrm(k):
        return rng.standard_normal((k, n))

    def axis(k, sign):
        x = np.zeros((k, n))
        x[:, b] = sign * (np.abs(rng.standard_normal(k)) + 0.1)
        return x

    p = {'normal': nrm(400), 'zero': np.zeros((40, n)), '+c e_b': axis(100, 1.0), '-c e_b': axis(100, -1.0)}
    z = nrm(160)
    z[:, b] = 0.0
    p['zero at b'] = z
    o = 1e-7 * nrm(200)
    o[np.arange(200), rng.integers(0, n, 200)] = rng.standard_normal(200) + 2.0
    p['one O(1), rest 1e-7'] = o
    p[f'tiny 2^{TINY[dn]}'] = np.ldexp(nrm(200), TINY[dn])
    return _assemble(p, NP[dn], rng)


@functools.lru_cache(maxsize=None)
def pairs(dn):
    """(x, y, cells): NB pairs for givens"""
    rng = np.random.default_rng(8500 + (dn == 'f64'))
    sc = np.where(np.arange(150) % 2 == 0, 1.0, 2.0 ** TINY[dn])      # every other axis-aligned pair is tiny
    ax = rng.standard_normal(150) * sc
    ay = rng.standard_normal(150) * sc
    r = rng.standard_normal((200, 2))
    r[np.arange(200), np.arange(200) % 2] *= 1e-6
    p = {'normal': rng.standard_normal((400, 2)), 'axis x': np.stack([ax, 0 * ax], -1),
         'axis y': np.stack([0 * ay, ay], -1), 'zero': np.zeros((50, 2)), 'ratio 1e-6': r,
         f'tiny 2^{TINY[dn]}': np.ldexp(rng.standard_normal((250, 2)), TINY[dn])}
    xy, cells = _assemble(p, NP[dn], rng)
    return _frozen(np.ascontiguousarray(xy[:, 0])), _frozen(np.ascontiguousarray(xy[:, 1])), cells


N_IDENTITY = 50        # the first records of `operands` carry u = 0 and (c, s) = (1, 0)


@functools.lru_cache(maxsize=None)
def operands(dn, n):
    """what the apply operations are fed besides matrices(dn, n): a unit reflector `u` of length n, a list `us` of
    reflectors of lengths n-1, n-2, .. 2 (the shape hessenberg returns), rotations (c, s) of shape (NB, 1), and a
    general matrix `m` for rq_hessenberg's u.  Rounded to the dtype: the judges use them as they are."""
    rng = np.random.default_rng(8700 + 100 * (dn == 'f64') + n)

    def unit(m):
        v = rng.standard_normal((NB, m))
        v /= np.sqrt((v * v).sum(-1, keepdims=True))
        v[:N_IDENTITY] = 0.0
        return _frozen(v.astype(NP[dn]))

    th = rng.uniform(0, 2 * np.pi, (NB, 1))
    c, s = np.cos(th), np.sin(th)
    c[:N_IDENTITY], s[:N_IDENTITY] = 1.0, 0.0
    return dict(u=unit(n), us=tuple(unit(n - 1 - k) for k in range(max(n - 2, 0))), c=_frozen(c.astype(NP[dn])),
                s=_frozen(s.astype(NP[dn])), m=_frozen(rng.standard_normal((NB, n, n)).astype(NP[dn])))


def ends(n):
    """the (i, j) of givens_apply: both ends, in both orders"""
    return ((0, n - 1), (n - 1, 0)) if n > 1 else ()


def sym_read(x, upper):
    """the symmetric matrix hessenberg_sym sees: one triangle of x, mirrored"""
    if upper:
        return np.triu(x) + np.triu(x, 1).swapaxes(-1, -2)
    return np.tril(x) + np.tril(x, -1).swapaxes(-1, -2)


# ------------------------------------------------------------------------------------------------ the operations
def inputs(dn, n):
    """everything run_all feeds the operations: a, hz, v{b}, x, y and the operands"""
    x, y, _ = pairs(dn)
    inp = dict(a=matrices(dn, n)[0], hz=hessenbergs(dn, n), x=x, y=y, **operands(dn, n))
    for b in sorted({0, n - 1}):
        inp[f'v{b}'] = vectors(dn, n, b)[0]
    return inp


def run_all(B, dn, n, inp=None):
    """every operation of backend B (the oracle's call shapes) on the batch (or on `inp`, a modified copy of
    inputs(dn, n)): {operation: [arrays]}"""
    ops = inp = inputs(dn, n) if inp is None else inp
    a, hz = inp['a'], inp['hz']
    out = {}
    for b in sorted({0, n - 1}):
        out[f'householder b={b}'] = list(B.householder(inp[f'v{b}'], b))
    out['givens'] = list(B.givens(inp['x'], inp['y']))
    out['hessenberg'] = [B.hessenberg(a)]
    h, us = B.hessenberg(a, True)
    out['hessenberg u'] = [h, *us]
    for up in (True, False):
        tri = 'upper' if up else 'lower'
        out[f'hessenberg_sym {tri}'] = [B.hessenberg_sym(a, upper=up)]
        h, us = B.hessenberg_sym(a, upper=up, compute_u=True)
        out[f'hessenberg_sym {tri} u'] = [h, *us]
        out[f'hessenberg_sym {tri} nofill'] = [B.hessenberg_sym(a, upper=up, fill=False)]
    out['qr_hessenberg'] = list(B.qr_hessenberg(hz))
    out['rq_hessenberg'] = [B.rq_hessenberg(hz)]
    out['rq_hessenberg u'] = list(B.rq_hessenberg(hz, ops['m']))
    for side in SIDES:
        out[f'householder_apply {side}'] = [B.householder_apply(a, ops['u'], side)]
    if n > 2:
        out['householder_apply list'] = [B.householder_apply(a, list(ops['us']), 'both')]
        out['householder_apply list inverse'] = [B.householder_apply(a, list(ops['us']), 'left', True)]
    for side in SIDES:
        for i, j in ends(n):
            out[f'givens_apply {side} {i},{j}'] = [B.givens_apply(a, ops['c'], ops['s'], i, j, side)]
    return out


def cells_of(op, dn, n):
    """{family: indices} of the batch an operation ran on"""
    if op.startswith('householder b='):
        return vectors(dn, n, int(op.split('=')[1]))[1]
    if op == 'givens':
        return pairs(dn)[2]
    return matrices(dn, n)[1]


# ------------------------------------------------------------------------------------------------ judges
def _ratio(err, den):
    """err / den per record; 0 / 0 = 0, x / 0 = inf, anything non-finite = inf"""
    err = np.asarray(err, HI)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return np.where(err <= 0, 0.0, np.where(den > 0, err / den, np.inf)).astype(np.float64)


def _exact(ok):
    return np.where(ok, 0.0, np.inf)


def _fro(x):
    x = np.asarray(x, HI).reshape(len(x), -1)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.sqrt((x * x).sum(-1))


def _finite(*arrs):
    return np.logical_and.reduce([np.isfinite(x.reshape(len(x), -1)).all(-1) for x in arrs])


def _gate(scores, fin):
    return {k: np.where(fin, v, np.inf) for k, v in scores.items()}


def _bits(x, y):
    """per record: x and y bit-identical (NaN positions included)"""
    same = (x == y) | (np.isnan(x) & np.isnan(y))
    return same.reshape(len(x), -1).all(-1)


def _mm(*ms):
    out = ms[0]
    for m in ms[1:]:
        out = np.einsum('bij,bjk->bik', out, m)
    return out


def _eye(n):
    return np.eye(n, dtype=HI)[None]


def reflector_matrix(u, n):
    """I - 2 w w^T in longdouble, w = u padded with leading zeros to length n (u as it is: not normalised)"""
    w = np.zeros((len(u), n), HI)
    if u.shape[-1]:
        w[:, n - u.shape[-1]:] = u
    return _eye(n) - 2 * w[:, :, None] * w[:, None, :]


def q_of(us, n, nb):
    """Q = P_0 P_1 ... of a reflector list"""
    q = np.broadcast_to(_eye(n), (nb, n, n)).copy()
    for u in us:
        q = _mm(q, reflector_matrix(u, n))
    return q


def judge_householder(dn, n, b, x, u, alpha):
    e = eps_of(dn)
    xh, uh, ah = x.astype(HI), u.astype(HI), alpha.astype(HI)
    nx = _fro(xh)
    px = xh - 2 * uh * (uh * xh).sum(-1, keepdims=True)
    px[:, b] -= ah
    zero = nx == 0
    xb = x[:, b]
    sign_ok = np.where(zero, True, np.where(xb > 0, alpha < 0, alpha > 0))
    s = {'reflects': _ratio(_fro(px), n * e * nx), 'alpha': _ratio(np.abs(np.abs(ah) - nx), n * e * nx),
         'unit': np.where(zero, 0.0, _ratio(np.abs(_fro(uh) - 1), e)),
         'zero exact': _exact(~zero | ((u == 0).all(-1) & (alpha == 0))), 'sign': _exact(sign_ok)}
    return _gate(s, _finite(u, alpha[:, None]))


def judge_givens(dn, x, y, c, s):
    e, n = eps_of(dn), 2
    xh, yh, ch, sh = (v.astype(HI) for v in (x, y, c, s))
    r = np.sqrt(xh * xh + yh * yh)
    want_c = np.where(y == 0, np.where(x == 0, 1.0, np.sign(x)), np.where(x == 0, 0.0, c))
    want_s = np.where(y == 0, 0.0, np.where(x == 0, -np.sign(y), s))
    sc = {'unit': _ratio(np.abs(ch * ch + sh * sh - 1), n * e), 'annihilates': _ratio(np.abs(sh * xh + ch * yh), n * e * r),
          'r': _ratio(np.abs(ch * xh - sh * yh - r), n * e * r), 'axis exact': _exact((c == want_c) & (s == want_s))}
    return _gate(sc, _finite(c[:, None], s[:, None]))


def _similarity(dn, n, a, h, us):
    """|Q H Q^T - A| / (n eps |A|)"""
    q = q_of(us, n, len(a))
    ah = a.astype(HI)
    return _ratio(_fro(_mm(q, h.astype(HI), q.swapaxes(-1, -2)) - ah), n * eps_of(dn) * _fro(ah))


def judge_hessenberg(dn, n, a, h, h_u, us, cells):
    s = {'similarity': _similarity(dn, n, a, h_u, us), 'structure': _exact((np.tril(h_u, -2) == 0).all((-1, -2))),
         'same without u': _exact(_bits(h, h_u))}
    back = np.ones(len(a), bool)
    for fam in ('zero', 'diagonal'):
        idx = cells[fam]
        back[idx] = (h_u[idx] == a[idx]).all((-1, -2))
    s['comes back'] = _exact(back)
    return _gate(s, _finite(h, h_u, *us))


def judge_hessenberg_sym(dn, n, a, upper, h, h_u, us, h_nofill, cells):
    sym = sym_read(a, upper)
    tri = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 1
    read = np.triu(np.ones((n, n), bool)) if upper else np.tril(np.ones((n, n), bool))
    s = {'similarity': _similarity(dn, n, sym, h_u, us),
         'structure': _exact((h_u[:, ~tri] == 0).all(-1) & (h_u == h_u.swapaxes(-1, -2)).all((-1, -2))),
         'same without u': _exact(_bits(h, h_u)),
         'nofill': _exact(_bits(h_nofill[:, read], h_u[:, read]) & _bits(h_nofill[:, ~read], a[:, ~read]))}
    back = np.ones(len(a), bool)
    for fam in ('zero', 'diagonal'):
        idx = cells[fam]
        back[idx] = (h_u[idx] == sym[idx]).all((-1, -2))
    s['comes back'] = _exact(back)
    return _gate(s, _finite(h, h_u, h_nofill, *us))


def judge_qr_hessenberg(dn, n, hz, q, r):
    e = eps_of(dn)
    hh, qh, rh = hz.astype(HI), q.astype(HI), r.astype(HI)
    nh = _fro(hh)
    s = {'Q R = H': _ratio(_fro(_mm(qh, rh) - hh), n * e * nh),
         'orthogonality': _ratio(_fro(_mm(qh.swapaxes(-1, -2), qh) - _eye(n)), n * e),
         'R triangular': _ratio(_fro(np.tril(rh, -1)), n * e * nh)}
    return _gate(s, _finite(q, r))


def judge_rq_hessenberg(dn, n, hz, q, r, rq, rq2, m2, m):
    """q, r: the same backend's qr_hessenberg(hz); rq = rq_hessenberg(hz); (rq2, m2) = rq_hessenberg(hz, m)"""
    e = eps_of(dn)
    hh, qh, rh, gh, mh = (v.astype(HI) for v in (hz, q, r, rq, m))
    nh = _fro(hh)
    s = {'RQ = r q': _ratio(_fro(gh - _mm(rh, qh)), n * e * nh),
         'q RQ q^T = H': _ratio(_fro(_mm(qh, gh, qh.swapaxes(-1, -2)) - hh), 2 * n * e * nh),
         "u' = u q": _ratio(_fro(m2.astype(HI) - _mm(mh, qh)), n * e * _fro(mh)), 'same with u': _exact(_bits(rq, rq2))}
    return _gate(s, _finite(q, r, rq, rq2, m2))


def _identity_rows(got, a):
    keep = np.ones(len(a), bool)
    keep[:N_IDENTITY] = _bits(got[:N_IDENTITY], a[:N_IDENTITY])
    return _exact(keep)


def judge_householder_apply(dn, n, a, us, side, inverse, got):
    ah = a.astype(HI)
    want = ah
    for u in (us[::-1] if inverse else us):
        p = reflector_matrix(u, n)
        if side in ('left', 'both'):
            want = _mm(p, want)
        if side in ('right', 'both'):
            want = _mm(want, p)
    s = {'product': _ratio(_fro(got.astype(HI) - want), n * eps_of(dn) * _fro(ah)), 'u = 0 exact': _identity_rows(got, a)}
    return _gate(s, _finite(got))


def rotation_matrix(c, s, i, j, n):
    """G with (row_i, row_j) <- (c row_i - s row_j, c row_j + s row_i): `left` is G A, `right` is A G^T"""
    g = np.broadcast_to(_eye(n), (len(c), n, n)).copy()
    ch, sh = c.astype(HI)[:, 0], s.astype(HI)[:, 0]
    g[:, i, i], g[:, i, j], g[:, j, i], g[:, j, j] = ch, -sh, sh, ch
    return g


def judge_givens_apply(dn, n, a, c, s, i, j, side, got):
    ah = a.astype(HI)
    g = rotation_matrix(c, s, i, j, n)
    want = ah
    if side in ('left', 'both'):
        want = _mm(g, want)
    if side in ('right', 'both'):
        want = _mm(want, g.swapaxes(-1, -2))
    sc = {'product': _ratio(_fro(got.astype(HI) - want), n * eps_of(dn) * _fro(ah)),
          '(1, 0) exact': _identity_rows(got, a)}
    return _gate(sc, _finite(got))


def score(dn, n, res):
    """{(operation, metric): per-record ratios} of `res` = run_all(B, dn, n)"""
    (a, cells), hz, ops = matrices(dn, n), hessenbergs(dn, n), operands(dn, n)
    out = {}

    def put(op, scores):
        out.update({(op, m): v for m, v in scores.items()})

    for b in sorted({0, n - 1}):
        op = f'householder b={b}'
        put(op, judge_householder(dn, n, b, vectors(dn, n, b)[0], *res[op]))
    x, y, _ = pairs(dn)
    put('givens', judge_givens(dn, x, y, *res['givens']))
    hu = res['hessenberg u']
    put('hessenberg', judge_hessenberg(dn, n, a, res['hessenberg'][0], hu[0], hu[1:], cells))
    for up in (True, False):
        op = f'hessenberg_sym {"upper" if up else "lower"}'
        hu = res[op + ' u']
        put(op, judge_hessenberg_sym(dn, n, a, up, res[op][0], hu[0], hu[1:], res[op + ' nofill'][0], cells))
    q, r = res['qr_hessenberg']
    put('qr_hessenberg', judge_qr_hessenberg(dn, n, hz, q, r))
    put('rq_hessenberg', judge_rq_hessenberg(dn, n, hz, q, r, res['rq_hessenberg'][0], *res['rq_hessenberg u'], ops['m']))
    for side in SIDES:
        op = f'householder_apply {side}'
        put(op, judge_householder_apply(dn, n, a, [ops['u']], side, False, res[op][0]))
    if n > 2:
        put('householder_apply list', judge_householder_apply(dn, n, a, list(ops['us']), 'both', False,
                                                              res['householder_apply list'][0]))
        put('householder_apply list inverse', judge_householder_apply(dn, n, a, list(ops['us']), 'left', True,
                                                                      res['householder_apply list inverse'][0]))
    for side in SIDES:
        for i, j in ends(n):
            op = f'givens_apply {side} {i},{j}'
            put(op, judge_givens_apply(dn, n, a, ops['c'], ops['s'], i, j, side, res[op][0]))
    return out


def worst(dn, n, scores):
    """{(operation, family): (worst ratio over the family's records and the operation's metrics, that metric)}"""
    out = {}
    for (op, m), v in scores.items():
        for fam, idx in cells_of(op, dn, n).items():
            w = float(v[idx].max())
            if (op, fam) not in out or w > out[(op, fam)][0]:
                out[(op, fam)] = (w, m)
    return out


def report(tag, dn, n, w):
    """one line per (operation, family), printed before anything is asserted"""
    for (op, fam), (ratio, m) in w.items():
        print(f'qr-family | {tag} | {dn} | {n} | {op} | {fam} | {ratio:.3g} | {m}')


def exceeding(w, bar=C):
    return {k: v for k, v in w.items() if not v[0] <= bar}


# ------------------------------------------------------------------------------------------------ orders 9..16
LARGE_ORDERS = (9, 12, 16)


@functools.lru_cache(maxsize=None)
def tiny_batch(dn, n):
    """the `tiny rows` family at any order, 64 records per shift, 64 `tiny border` records at the largest shift and 13
    normal ones (397: no multiple of 64), shuffled.  Returns (a, cells)"""
    rng = np.random.default_rng(8900 + 100 * (dn == 'f64') + n)
    p = {'normal': rng.standard_normal((13, n, n))}
    for s in TINY_SHIFTS[dn]:
        t = rng.standard_normal((64, n, n))
        t[:, 2:, :] = np.ldexp(t[:, 2:, :], -s)
        p[f'tiny rows 2^-{s}'] = t
    p[f'tiny border 2^-{TINY_SHIFTS[dn][-1]}'] = tiny_border(rng.standard_normal((64, n, n)), TINY_SHIFTS[dn][-1])
    with np.errstate(under='ignore'):
        a = np.concatenate(list(p.values())).astype(NP[dn])
    perm = rng.permutation(len(a))
    where = np.empty(len(a), np.int64)
    where[perm] = np.arange(len(a))
    cells, at = {}, 0
    for name, x in p.items():
        cells[name] = _frozen(np.sort(where[at:at + len(x)]))
        at += len(x)
    assert len(a) % 64 != 0
    return _frozen(a[perm]), cells


def tiny_vectors(dn, n):
    """column 0 of the tiny batch below the diagonal, padded with its last entry to length n: the vectors
    hessenberg reflects first, tiny ones and O(1) ones in one wavefront"""
    a = tiny_batch(dn, n)[0]
    return np.ascontiguousarray(np.concatenate([a[:, 1:, 0], a[:, -1:, 0]], -1))


def run_tiny(B, dn, n):
    a = tiny_batch(dn, n)[0]
    hz = np.triu(a, -1)
    h, us = B.hessenberg(a, True)
    out = {'hessenberg u': [h, *us], 'qr_hessenberg': list(B.qr_hessenberg(hz)), 'rq_hessenberg': [B.rq_hessenberg(hz)]}
    for up in (True, False):
        h, us = B.hessenberg_sym(a, upper=up, compute_u=True)
        out[f'hessenberg_sym {"upper" if up else "lower"} u'] = [h, *us]
    for b in (0, n - 1):
        out[f'householder b={b}'] = list(B.householder(tiny_vectors(dn, n), b))
    return out


def worst_tiny(dn, n, res):
    """{(operation, family): (worst ratio, metric)} of run_tiny's results"""
    a, cells = tiny_batch(dn, n)
    hu = res['hessenberg u']
    sc = {('hessenberg', 'similarity'): np.where(_finite(*hu), _similarity(dn, n, a, hu[0], hu[1:]), np.inf),
          ('hessenberg', 'structure'): _exact((np.tril(hu[0], -2) == 0).all((-1, -2)))}
    hz = np.triu(a, -1)
    q, r = res['qr_hessenberg']
    sc.update({('qr_hessenberg', m): v for m, v in judge_qr_hessenberg(dn, n, hz, q, r).items()})
    rq = res['rq_hessenberg'][0]
    rqs = judge_rq_hessenberg(dn, n, hz, q, r, rq, rq, a, a)
    sc.update({('rq_hessenberg', m): rqs[m] for m in ('RQ = r q', 'q RQ q^T = H')})
    tri = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 1
    for up in (True, False):
        hu = res[f'hessenberg_sym {"upper" if up else "lower"} u']
        op = f'hessenberg_sym {"upper" if up else "lower"}'
        sc[(op, 'similarity')] = np.where(_finite(*hu), _similarity(dn, n, sym_read(a, up), hu[0], hu[1:]), np.inf)
        sc[(op, 'structure')] = _exact((hu[0][:, ~tri] == 0).all(-1))
    for b in (0, n - 1):
        sc.update({(f'householder b={b}', m): v
                   for m, v in judge_householder(dn, n, b, tiny_vectors(dn, n), *res[f'householder b={b}']).items()})
    out = {}
    for (op, m), v in sc.items():
        for fam, idx in cells.items():
            w = float(v[idx].max())
            if (op, fam) not in out or w > out[(op, fam)][0]:
                out[(op, fam)] = (w, m)
    return out


@functools.lru_cache(maxsize=None)
def oracle_results(oracle, dn, n):
    """the oracle on the batch, once, frozen"""
    res = run_all(oracle, dn, n)
    for arrs in res.values():
        for x in arrs:
            x.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ bit identity
def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and bool(np.array_equal(x, y, equal_nan=True))


def differing(got, ref):
    """{operation: indices of the records that differ in any array}; empty where bit-identical"""
    assert got.keys() == ref.keys(), (sorted(got), sorted(ref))
    out = {}
    for op in ref:
        assert len(got[op]) == len(ref[op]), op
        bad = np.zeros(len(ref[op][0]), bool)
        for x, y in zip(got[op], ref[op]):
            assert x.shape == y.shape and x.dtype == y.dtype, (op, x.shape, y.shape, x.dtype, y.dtype)
            bad |= ~_bits(x, y)
        if bad.any():
            out[op] = np.flatnonzero(bad)
    return out


def families_of(op, dn, n, idx):
    """the families the records `idx` of an operation belong to"""
    return sorted(f for f, c in cells_of(op, dn, n).items() if np.intersect1d(c, idx).size)
