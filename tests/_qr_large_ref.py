"""Inputs, storage forms and assertions of the QR family at orders 9..16 (shared by
test_qr_large_orders_host.py, which holds the ORACLE to every bar below, and test_gpu_qr_large_orders.py,
which holds the kernels to them).

Every bar is one that tests/test_gpu_qr.py::test_vs_oracle already makes at n in {9, 12, 16}: TOL against
the oracle, `check_eigenpairs`, `within_model` against numpy.linalg.eigvalsh in float64, Q R = H to
16 n eps |H|, P x = alpha e_b to 16 n eps |x|.  Nothing here is a new number.

Inputs are built once per (dtype, order) and frozen; a backend is anything with the oracle's call shapes
(the `oracle` module itself, or `GpuQ` of test_gpu_qr.py)."""
import functools
import numpy as np
import torch
from conftest import TOL, EPS, relerr, within_model
from _solver_ref import per_matrix_err

NP = {'f32': np.float32, 'f64': np.float64}
ORDERS = tuple(range(9, 17))
# the register / LDS switch-over orders of nfm_qr.hip (NFM_QRL_*_MAX and the order after each) and both ends
VOTE_ORDERS = (9, 10, 11, 13, 15, 16)
SIDES = ('left', 'right', 'both')
# (input, upper): the symmetrised records, and the general ones read from either triangle (a symmetric input
# would not notice a kernel that reads the wrong one)
EIG_CASES = (('sym', True), ('a', True), ('a', False))
# seed of the records of a (dtype, order): 2000 + n unless the oracle alone misses a bar there (none does)
SEEDS = {}


def nb_of(n):
    """more than fifteen full workgroups of 64 or 32 lanes and a ragged last one, never a multiple of 64"""
    return 1000 + n


def _frozen(d):
    for x in d.values():
        x.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def records(dn, n):
    """N(0, 1) general matrices `a`, their symmetrised versions `sym`, Hessenberg matrices `hz` and vectors `v`"""
    rng = np.random.default_rng(SEEDS.get((dn, n), 2000 + n))
    nb = nb_of(n)
    a = rng.standard_normal((nb, n, n)).astype(NP[dn])
    sym = ((a + a.transpose(0, 2, 1)) / 2).astype(NP[dn])
    v = rng.standard_normal((nb, n)).astype(NP[dn])
    return _frozen(dict(a=a, sym=sym, hz=np.triu(a, -1), v=v))


def eig_tag(key, upper):
    return f'{key} {"upper" if upper else "lower"}'


def sym_read(x, upper):
    """the symmetric matrix eig_sym / hessenberg_sym see: one triangle of x, mirrored"""
    if upper:
        return np.triu(x) + np.triu(x, 1).transpose(0, 2, 1)
    return np.tril(x) + np.tril(x, -1).transpose(0, 2, 1)


@functools.lru_cache(maxsize=None)
def eig_truth(dn, n):
    """numpy.linalg.eigvalsh in float64 of every EIG_CASES input (ascending)"""
    r = records(dn, n)
    return {eig_tag(k, up): np.linalg.eigvalsh(sym_read(r[k], up).astype(np.float64)) for k, up in EIG_CASES}


@functools.lru_cache(maxsize=None)
def aux(oracle, dn, n):
    """what the apply operations are fed: the oracle's reflector of `v`, its reflector list of
    hessenberg(a, compute_u=True) and a rotation from givens -- so that only the apply is compared"""
    r = records(dn, n)
    c, s = oracle.givens(r['v'][:, 0], r['v'][:, 1])
    return dict(hh_u=oracle.householder(r['v'], 0)[0], hess_us=tuple(oracle.hessenberg(r['a'], True)[1]),
                c=np.ascontiguousarray(c[:, None]), s=np.ascontiguousarray(s[:, None]))


@functools.lru_cache(maxsize=None)
def oracle_family(oracle, dn, n):
    """the oracle's results of every reference-order operation, computed once: (eig_family, rest_family)"""
    r = records(dn, n)
    eig, rest = eig_family(oracle, r), rest_family(oracle, r, aux(oracle, dn, n), n)
    for arrs in (*eig.values(), *rest.values()):
        for x in arrs:
            x.setflags(write=False)
    return eig, rest


# ------------------------------------------------------------------------------------------ the operations
def eig_family(B, r):
    """eig_sym of backend B, values and values + vectors, for every EIG_CASES input: {operation: [arrays]}"""
    out = {}
    for key, up in EIG_CASES:
        out['eig_sym ' + eig_tag(key, up)] = [B.eig_sym(r[key], upper=up)]
        out['eig_sym vectors ' + eig_tag(key, up)] = list(B.eig_sym(r[key], compute_u=True, upper=up))
    return out


def rest_family(B, r, ax, n):
    """every other operation of the family: {operation: [arrays]}"""
    a, hz, v = r['a'], r['hz'], r['v']
    out = {'hessenberg': [B.hessenberg(a)]}
    h, us = B.hessenberg(a, True)
    out['hessenberg reflectors'] = [h, *us]
    for up in (True, False):
        tri = 'upper' if up else 'lower'
        out['hessenberg_sym ' + tri] = [B.hessenberg_sym(a, upper=up)]
        h, us = B.hessenberg_sym(a, upper=up, compute_u=True)
        out['hessenberg_sym reflectors ' + tri] = [h, *us]
    out['qr_hessenberg'] = list(B.qr_hessenberg(hz))
    out['rq_hessenberg'] = [B.rq_hessenberg(hz)]
    out['rq_hessenberg u'] = list(B.rq_hessenberg(hz, a))
    for b in (0, n - 1):
        out[f'householder basis {"0" if b == 0 else "n-1"}'] = list(B.householder(v, b))
    for side in SIDES:
        out['householder_apply ' + side] = [B.householder_apply(a, ax['hh_u'], side)]
    out['householder_apply inverse'] = [B.householder_apply(a, list(ax['hess_us']), 'left', True)]
    for side in SIDES:
        out['givens_apply ' + side] = [B.givens_apply(a, ax['c'], ax['s'], 0, n - 1, side)]
    return out


def same_bits(x, y):
    """NaN positions included"""
    return x.shape == y.shape and x.dtype == y.dtype and bool(np.array_equal(x, y, equal_nan=True))


def family_bits(got, ref):
    """{operation: every array bit-identical}"""
    assert got.keys() == ref.keys()
    return {op: len(got[op]) == len(ref[op]) and all(same_bits(x, y) for x, y in zip(got[op], ref[op])) for op in ref}


def worst_record(x, y):
    e = per_matrix_err(np.nan_to_num(x, nan=np.inf), y)
    return int(np.argmax(e)), float(e.max())


def check_tol(got, ref, dn, emit=None):
    """every array of every operation within TOL of the reference's, batch max-norm; `emit(operation, worst
    relerr, bit-identical)` once per operation"""
    bits = family_bits(got, ref)
    for op, arrs in ref.items():
        errs = [relerr(x, y) for x, y in zip(got[op], arrs)]
        if emit is not None:
            emit(op, max(errs), bits[op])
        for k, (x, y, e) in enumerate(zip(got[op], arrs, errs)):
            assert e <= TOL[dn], (op, k, e, worst_record(x, y))


def check_eig(got, ref, dn, n, fast=False):
    """eig_sym results `got` against the reference-order oracle results `ref` and the float64 truth: the sorted
    values within the error model, eigenpairs by their defining equations (test_vs_oracle's assertions)"""
    from test_gpu_qr import check_eigenpairs
    r, truth = records(dn, n), eig_truth(dn, n)
    for key, up in EIG_CASES:
        tag = eig_tag(key, up)
        rv = np.sort(ref['eig_sym ' + tag][0], -1)
        for op in ('eig_sym ' + tag, 'eig_sym vectors ' + tag):
            ev = np.sort(got[op][0], -1)
            assert within_model(ev, rv, truth[tag], n, dn), (op, fast, relerr(ev, truth[tag]))
        ev, evec = got['eig_sym vectors ' + tag]
        check_eigenpairs(sym_read(r[key], up), ev, evec, n, dn)


def check_relations(got, ref, dn, n):
    """Q R = H, R Q, P x = alpha e_b (test_vs_oracle's), on `got`'s own factors"""
    r = records(dn, n)
    hz, v = r['hz'], r['v'].astype(np.float64)
    q, rr = (x.astype(np.float64) for x in got['qr_hessenberg'])
    assert np.abs(np.einsum('bij,bjk->bik', q, rr) - hz).max() <= 16 * n * EPS[dn] * np.abs(hz).max()
    qo, ro = (x.astype(np.float64) for x in ref['qr_hessenberg'])
    assert relerr(got['rq_hessenberg'][0], np.einsum('bij,bjk->bik', ro, qo)) <= 4 * n * EPS[dn] + TOL[dn]
    for b in (0, n - 1):
        u, al = got[f'householder basis {"0" if b == 0 else "n-1"}']
        u = u.astype(np.float64)
        px = v - 2 * u * (u * v).sum(-1, keepdims=True)
        e = np.zeros_like(v)
        e[:, b] = al
        assert np.abs(px - e).max() <= 16 * n * EPS[dn] * np.abs(v).max(), (b, np.abs(px - e).max())


# ------------------------------------------------------------------------------------------ storage forms
TWO_LEVEL = (3, 340, 337)          # torch.zeros(3, 340, ...)[:, :337]: n_outer = 3, a ragged last tile in every slab
FORMS = ('matrix-first', 'two-level')


def two_level_index(nb):
    """records of the two-level batch: the first 3 * 337 = 1011 (orders 9 and 10 have 1009 and 1010 records:
    the batch wraps around to records 0 and 1)"""
    return np.arange(TWO_LEVEL[0] * TWO_LEVEL[2]) % nb


def present(x, form):
    """the batch-first tensor x (nb, ...) as a view that the register form of orders 9..16 does not take:
    'matrix-first': (..., nb) contiguous storage viewed as (nb, ...), batch stride 1;
    'two-level':    contiguous records in a (3, 340, ...) buffer of which [:, :337] is used"""
    if form == 'contiguous':
        return x.contiguous()
    if form == 'matrix-first':
        return x.movedim(0, -1).contiguous().movedim(-1, 0)
    assert form == 'two-level'
    no, pitch, ni = TWO_LEVEL
    idx = torch.from_numpy(two_level_index(len(x))).to(x.device)
    view = torch.zeros((no, pitch) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)[:, :ni]
    view.copy_(x[idx].reshape((no, ni) + tuple(x.shape[1:])))
    return view


def as_batch_first(res, form):
    """results of a `form` call as (records, ...) arrays"""
    if form != 'two-level':
        return res
    return {op: [x.reshape((-1,) + x.shape[2:]) for x in arrs] for op, arrs in res.items()}


def expected_of(res, form, nb):
    """what a `form` call must return, from the contiguous call's results"""
    if form != 'two-level':
        return res
    idx = two_level_index(nb)
    return {op: [x[idx] for x in arrs] for op, arrs in res.items()}


# ------------------------------------------------------------------------------------------ range votes
@functools.lru_cache(maxsize=None)
def vote_batch(dn, n):
    """the batch of test_gpu_qr.py::test_eig_sym_default_bits_across_ranges at order n: whole wavefronts at one
    scale, eight wavefronts mixing the scales lane by lane, 16 diagonal, 8 zero, 16 block-diagonal records and 8
    of denormal-sized entries (the rest: unit scale).  Returns (a, k, ex): k the index of the first diagonal record"""
    dtype = NP[dn]
    rng = np.random.default_rng(500 + n)
    nb = 64 * 40
    a = rng.standard_normal((nb, n, n))
    a = a + a.swapaxes(-1, -2)
    ex = (-30, -20, -14, -8, 0, 5, 8, 12, 18) if dn == 'f32' else (-250, -190, -120, -40, 0, 20, 45, 70, 140)
    scale = np.ones(nb)
    for i, e in enumerate(ex):                      # whole wavefronts at one scale ...
        scale[64 * i:64 * (i + 1)] = 10.0 ** e
    mixed = slice(64 * len(ex), 64 * (len(ex) + 8))   # ... and wavefronts that mix the scales lane by lane
    scale[mixed] = 10.0 ** rng.choice(ex, size=64 * 8)
    a = a * scale[:, None, None]
    k = 64 * (len(ex) + 8)
    a[k:k + 16] = np.eye(n) * rng.standard_normal((16, 1, n))           # diagonal
    a[k + 16:k + 24] = 0.0                                                # zero
    a[k + 24:k + 40, 0, 1:] = 0.0                                         # block diagonal: exact zeros off the blocks
    a[k + 24:k + 40, 1:, 0] = 0.0
    tiny = np.finfo(dtype).tiny
    a[k + 40:k + 48] = rng.standard_normal((8, n, n)) * tiny * 4          # denormal-sized entries
    a[k + 40:k + 48] += a[k + 40:k + 48].swapaxes(-1, -2).copy()
    a = a.astype(dtype)
    a.setflags(write=False)
    return a, k, ex


def vote_nonfinite(a):
    """the NaN / inf pattern of that test on the first 256 records"""
    b = a[:256].copy()
    b[::7, 0, 0] = np.nan
    b[3::11, -1, 0] = np.inf
    b[3::11, 0, -1] = np.inf
    return b


def vote_fast_subset(dn, n):
    """what arithmetic='fast' is run on: the unit-scale wavefront and the diagonal, zero and block-diagonal
    records.  Returns (records, slice of the diagonal ones, slice of the zero ones)"""
    a, k, ex = vote_batch(dn, n)
    unit = ex.index(0)
    return np.concatenate([a[64 * unit:64 * (unit + 1)], a[k:k + 40]]), slice(64, 80), slice(80, 88)


@functools.lru_cache(maxsize=None)
def vote_refs(oracle, dn, n):
    """the oracle on the vote batch, once: values, (values, vectors), values of the non-finite variant, values
    of the fast subset"""
    a = vote_batch(dn, n)[0]
    return oracle.eig_sym(a), oracle.eig_sym(a, True), oracle.eig_sym(vote_nonfinite(a)), \
        oracle.eig_sym(vote_fast_subset(dn, n)[0])


def check_fast_subset(vals, vals_u, vecs, ref_vals, dn, n, exact=True):
    """diagonal and zero records come back exact (test_eig_sym_nothing_left_to_iterate's assertion), the rest
    meets check_eigenpairs and within_model against the reference-order oracle values `ref_vals`.
    exact=False is for the oracle: the reference's sweeps shift a stage before they test it, and
    (d - sigma) + sigma moves a diagonal entry by an ulp -- its diagonal records are held to the model only."""
    from test_gpu_qr import check_eigenpairs
    sub, diag, zero = vote_fast_subset(dn, n)
    want = np.sort(np.diagonal(sub[diag], axis1=1, axis2=2), -1)
    truth = np.linalg.eigvalsh(sub.astype(np.float64))
    for v in (vals, vals_u):
        if exact:
            assert np.array_equal(np.sort(v[diag], -1), want), np.abs(np.sort(v[diag], -1) - want).max()
        assert np.array_equal(v[zero], np.zeros_like(v[zero]))
        assert within_model(np.sort(v, -1), np.sort(ref_vals, -1), truth, n, dn), relerr(np.sort(v, -1), truth)
    check_eigenpairs(sub, vals_u, vecs, n, dn)
