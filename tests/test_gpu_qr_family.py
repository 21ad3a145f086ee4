"""The QR building blocks (givens, givens_apply, householder, householder_apply, hessenberg, hessenberg_sym,
qr_hessenberg, rq_hessenberg) at orders 1..8, the orders of the workload, held to the per-record bounds of
tests/_qr_ref.py on hard inputs, to the oracle bit for bit, and to their own contiguous call bit for bit in
every storage form the launcher of nfm_record_kernel.hpp distinguishes.  test_qr_family_host.py shows that the
oracle alone meets the same bounds on the same inputs.

Every test that judges prints its `qr-family` lines (worst ratio per operation and family) before it asserts;
profiles/qr_family_accuracy.md is assembled from them."""
import functools
import numpy as np
import pytest
import torch
from test_gpu_qr import Q, t, n_
import _qr_large_ref as L
import _qr_ref as R

pytestmark = pytest.mark.gpu
INT = {torch.float32: torch.int32, torch.float64: torch.int64}
DTYPES = ['f32', 'f64']
FORMS = ('matrix-first', 'two-level', 'every other', 'padded rows', 'padded records', 'offset', 'mT', 'real parts')


class G:
    """the building blocks on the GPU behind the oracle's call shapes (numpy in, numpy out); `kw` goes to every
    call that takes it (check_finite=False)"""

    def __init__(self, dev, **kw):
        self.dev, self.kw = dev, kw

    def t(self, x):
        return t(x, self.dev)

    def householder(self, v, basis=0):
        u, al = Q().householder(self.t(v), basis=basis, return_alpha=True, **self.kw)
        return n_(u), n_(al)

    def givens(self, x, y):
        c, s = Q().givens(self.t(x), self.t(y))
        return n_(c), n_(s)

    def householder_apply(self, a, u, side='both', inverse=False):
        u = [self.t(x) for x in u] if isinstance(u, list) else self.t(u)
        return n_(Q().householder_apply(self.t(a), u, side=side, inverse=inverse, **self.kw))

    def givens_apply(self, a, c, s, i=0, j=None, side='both'):
        return n_(Q().givens_apply(self.t(a), self.t(c), self.t(s), i, j, side=side, **self.kw))

    def hessenberg(self, a, compute_u=False):
        if compute_u:
            h, us = Q().hessenberg(self.t(a), compute_u=True, **self.kw)
            return n_(h), [n_(x) for x in us]
        return n_(Q().hessenberg(self.t(a), **self.kw))

    def hessenberg_sym(self, a, upper=True, fill=True, compute_u=False):
        r = Q().hessenberg_sym(self.t(a), upper=upper, fill=fill, compute_u=compute_u, **self.kw)
        return (n_(r[0]), [n_(x) for x in r[1]]) if compute_u else n_(r)

    def qr_hessenberg(self, h):
        q, r = Q().qr_hessenberg(self.t(h), **self.kw)
        return n_(q), n_(r)

    def rq_hessenberg(self, h, u=None):
        if u is None:
            return n_(Q().rq_hessenberg(self.t(h), **self.kw))
        h2, u2 = Q().rq_hessenberg(self.t(h), self.t(u), **self.kw)
        return n_(h2), n_(u2)


def present(x, form):
    """the batch-first tensor x (nb, ...) in one storage form; the padding of every buffer is NaN (a kernel that
    reads it shows)"""
    if form in ('contiguous', 'matrix-first', 'two-level'):
        return L.present(x, form)
    if form == 'mT':                                   # the matrix operand stored transposed
        return x.mT.contiguous().mT if x.dim() >= 3 else x.contiguous()
    nb, rest = x.shape[0], tuple(x.shape[1:])

    def nans(*shape):
        return torch.full(shape, float('nan'), dtype=x.dtype, device=x.device)

    if form == 'every other':
        view = nans(2 * nb, *rest)[::2]
    elif form == 'padded rows':
        view = nans(nb, *rest[:-1], rest[-1] + 3)[..., :rest[-1]] if rest else nans(nb, 3)[:, 0]
    elif form == 'padded records':
        rec = int(np.prod(rest, dtype=np.int64))
        inner = tuple(int(np.prod(rest[k + 1:], dtype=np.int64)) for k in range(len(rest)))
        view = nans(nb * (rec + 5)).as_strided((nb,) + rest, (rec + 5,) + inner)
    elif form == 'offset':                             # base one element off the allocation's alignment
        view = nans(x.numel() + 1)[1:].view(x.shape)
    else:
        assert form == 'real parts'                    # x[..., ::2] of a doubled last axis
        view = nans(nb, *rest[:-1], 2 * rest[-1])[..., ::2] if rest else nans(2 * nb)[::2]
    view.copy_(x)
    return view


def whole_buffer(view):
    """every byte of the allocation behind a view, padding included"""
    return torch.empty(0, dtype=torch.uint8, device=view.device).set_(view.untyped_storage())


class Form(G):
    """G whose operands reach the library in one storage form, and which keeps a copy of the whole buffer behind every
    view it hands out: `unchanged()` compares them byte for byte after the calls, the NaN padding included"""

    def __init__(self, dev, form, **kw):
        super().__init__(dev, **kw)
        self.form, self.seen = form, []

    def t(self, x):
        view = present(t(x, self.dev), self.form)
        self.seen.append((view, whole_buffer(view).clone()))
        return view

    def unchanged(self):
        ok = all(torch.equal(whole_buffer(v), c) for v, c in self.seen)
        self.seen = []
        return ok


@functools.lru_cache(maxsize=None)
def gpu_results(dev, dn, n):
    """the contiguous call of every operation on the batch, once, frozen"""
    res = R.run_all(G(dev), dn, n)
    for arrs in res.values():
        for x in arrs:
            x.setflags(write=False)
    return res


def describe(diff, dn, n):
    return {op: (len(idx), R.families_of(op, dn, n, idx)) for op, idx in diff.items()}


@pytest.mark.parametrize('dn', DTYPES)
@pytest.mark.parametrize('n', R.ORDERS)
def test_bounds(dev, dn, n):
    """every judge of _qr_ref on every family, the contiguous batch; no family is left out"""
    w = R.worst(dn, n, R.score(dn, n, gpu_results(dev, dn, n)))
    R.report('gpu', dn, n, w)
    assert {f for _, f in w} >= set(R.matrices(dn, n)[1]) | set(R.pairs(dn)[2]) | set(R.vectors(dn, n, 0)[1])
    assert not R.exceeding(w), R.exceeding(w)


@pytest.mark.parametrize('dn', DTYPES)
@pytest.mark.parametrize('n', R.ORDERS)
def test_oracle_parity_per_record(dev, oracle, dn, n):
    """on all families the kernels match the oracle bit for bit, record by record.  The kernels keep float32
    denormals (they are not flushed): the cells whose sums of squares hold subnormal terms agree as well"""
    diff = R.differing(gpu_results(dev, dn, n), R.oracle_results(oracle, dn, n))
    print(f'qr-family-parity | {dn} | {n} | {describe(diff, dn, n) or "bit-identical"}')
    assert not diff, describe(diff, dn, n)


@pytest.mark.parametrize('dn', DTYPES)
@pytest.mark.parametrize('n', R.ORDERS)
@pytest.mark.parametrize('form', FORMS)
def test_storage_forms(dev, dn, n, form):
    """every operation, every operand in one storage form: bit-identical to the contiguous call, inputs unchanged"""
    F = Form(dev, form)
    got = L.as_batch_first(R.run_all(F, dn, n), form)
    assert F.unchanged()
    diff = R.differing(got, L.expected_of(gpu_results(dev, dn, n), form, R.NB))
    assert not diff, {op: len(idx) for op, idx in diff.items()}


def _same(got, want):
    got = got if isinstance(got, (tuple, list)) else [got]
    want = want if isinstance(want, (tuple, list)) else [want]
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.shape == y.shape and torch.equal(x.view(INT[x.dtype]), y.view(INT[y.dtype]))


@pytest.mark.parametrize('dn', DTYPES)
@pytest.mark.parametrize('n', R.ORDERS)
def test_broadcast_operands(dev, dn, n):
    """a stride-0 broadcast of each operand in turn, for the operations with two operands: bit-identical to the call
    on the materialised operands"""
    inp = R.inputs(dn, n)
    a, hz, m, u, c, s = (t(inp[k], dev) for k in ('a', 'hz', 'm', 'u', 'c', 's'))
    x, y = t(inp['x'], dev), t(inp['y'], dev)
    one = 777                                           # the record that is broadcast
    full = lambda v: v[one].expand_as(v).contiguous()
    _same(Q().rq_hessenberg(hz, m[one]), Q().rq_hessenberg(hz, full(m)))
    _same(Q().rq_hessenberg(hz[one], m), Q().rq_hessenberg(full(hz), m))
    for side in R.SIDES:
        _same(Q().householder_apply(a, u[one], side=side), Q().householder_apply(a, full(u), side=side))
        _same(Q().householder_apply(a[one], u, side=side), Q().householder_apply(full(a), u, side=side))
        for i, j in R.ends(n):
            _same(Q().givens_apply(a, c[one], s[one], i, j, side=side), Q().givens_apply(a, full(c), full(s), i, j, side=side))
            _same(Q().givens_apply(a[one], c, s, i, j, side=side), Q().givens_apply(full(a), c, s, i, j, side=side))
    if n == R.ORDERS[0]:                                # givens has no order
        _same(Q().givens(x[one], y), Q().givens(full(x), y))
        _same(Q().givens(x, y[one]), Q().givens(x, full(y)))


BAD = (63, 64, 600)     # the last lane of a wavefront, the first of the next, mid-tile in the second tile


@pytest.mark.parametrize('dn', DTYPES)
@pytest.mark.parametrize('n', R.ORDERS)
def test_bad_records_leave_their_neighbours_alone(dev, dn, n):
    """a NaN record (check_finite=False), a zero record and a `tiny rows` record (for vectors and pairs: all tiny)
    at positions 63, 64 and 600 of every operand: every other record is bit-identical to the clean run"""
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else tuple(x.copy() for x in v)) for k, v in R.inputs(dn, n).items()}
    a, cells = R.matrices(dn, n)
    tiny_rec = a[cells[f'tiny rows 2^-{R.TINY_SHIFTS[dn][-1]}'][0]]
    for k, v in inp.items():
        for arr in (v if isinstance(v, tuple) else (v,)):
            arr[BAD[0]], arr[BAD[1]] = np.nan, 0.0
            arr[BAD[2]] = tiny_rec if arr.shape[1:] == tiny_rec.shape else np.ldexp(arr[BAD[2]], R.TINY[dn])
    inp['hz'] = np.triu(inp['hz'], -1)
    got = R.run_all(G(dev, check_finite=False), dn, n, inp)
    clean = gpu_results(dev, dn, n)
    diff = R.differing(got, clean)
    stray = {op: sorted(set(idx) - set(BAD)) for op, idx in diff.items() if set(idx) - set(BAD)}
    assert not stray, stray
    for op, arrs in got.items():                        # the zero and the tiny record themselves come out finite
        assert all(np.isfinite(x[[BAD[1], BAD[2]]]).all() for x in arrs), op


@pytest.mark.parametrize('dn', DTYPES)
@pytest.mark.parametrize('n', R.LARGE_ORDERS)
@pytest.mark.parametrize('form', ['contiguous', 'matrix-first'])
def test_tiny_rows_large_orders(dev, oracle, dn, n, form):
    """the `tiny rows` and `tiny border` families at orders 9, 12 and 16 through every guarded operation -- hessenberg,
    hessenberg_sym (both triangles), qr_hessenberg, rq_hessenberg, householder (both ends) -- contiguous (the register
    form where the order fits) and matrix-first (the LDS-resident form): both kernel forms of nfm_qr.hip carry the
    range guard -- the bounds, and the oracle bit for bit"""
    F = Form(dev, form)
    got = R.run_tiny(F, dn, n)
    assert F.unchanged()
    w = R.worst_tiny(dn, n, got)
    R.report(f'gpu {form}', dn, n, w)
    assert not R.exceeding(w), R.exceeding(w)
    diff = R.differing(got, R.run_tiny(oracle, dn, n))
    assert not diff, {op: len(idx) for op, idx in diff.items()}
