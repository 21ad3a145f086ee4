"""The reference side of test_gpu_qr_large_orders.py, without a GPU: the oracle alone meets every bar that
module holds the kernels to, on the same inputs, at every order 9..16 -- so a green GPU test never rests on
a bound the reference itself misses -- and the storage forms of that module reach the C ABI as the views
they are, uncopied.

No order needed another seed: the oracle meets every relation on the records of seed 2000 + n."""
import numpy as np
import pytest
import torch
from conftest import relerr
import _qr_large_ref as R


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.ORDERS)
def test_oracle_meets_the_bars(oracle, dn, n):
    r, ax = R.records(dn, n), R.aux(oracle, dn, n)
    assert len(r['a']) == R.nb_of(n) and len(r['a']) % 64 and len(r['a']) > 15 * 64
    assert all(x.dtype == R.NP[dn] for x in r.values())
    eig, rest = R.eig_family(oracle, r), R.rest_family(oracle, r, ax, n)
    for op, arrs in {**eig, **rest}.items():
        assert all(np.isfinite(x).all() for x in arrs), op
    # hessenberg's reflector k has length n - 1 - k, and there are n - 2 of them
    assert [u.shape[-1] for u in rest['hessenberg reflectors'][1:]] == list(range(n - 1, 1, -1))
    R.check_tol({**eig, **rest}, {**eig, **rest}, dn)
    R.check_eig(eig, eig, dn, n)
    R.check_relations(rest, rest, dn, n)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.VOTE_ORDERS)
def test_oracle_on_the_vote_batch(oracle, dn, n):
    """the batch of part 3: its structure (scales in and out of range inside one wavefront, exact zeros,
    denormal entries), and the oracle against the bars of the fast subset"""
    a, k, ex = R.vote_batch(dn, n)
    assert a.shape == (64 * 40, n, n) and np.isfinite(a).all()
    amax = np.abs(a).reshape(len(a), -1).max(-1)
    for w in range(len(ex), len(ex) + 8):           # every mixed wavefront spans the exponent range
        lanes = amax[64 * w:64 * (w + 1)]
        assert np.log10(lanes.max()) - np.log10(lanes.min()) > 30
    assert (a[k:k + 16] * (1 - np.eye(n)) == 0).all() and (a[k + 16:k + 24] == 0).all()
    assert (a[k + 24:k + 40, 0, 1:] == 0).all() and np.abs(a[k + 24:k + 40, 1:, 1:]).min() > 0
    assert 0 < np.abs(a[k + 40:k + 48]).max() < 64 * np.finfo(R.NP[dn]).tiny
    b = R.vote_nonfinite(a)
    ref = oracle.eig_sym(b)
    assert np.isnan(ref[::7]).any() and np.isfinite(ref).any()
    sub, diag, zero = R.vote_fast_subset(dn, n)
    assert sub.shape == (104, n, n)
    vals = oracle.eig_sym(sub)
    vals_u, vecs = oracle.eig_sym(sub, True)
    R.check_fast_subset(vals, vals_u, vecs, vals, dn, n, exact=False)


@pytest.mark.parametrize('n', [9, 16])
def test_forms_reach_the_c_abi_uncopied(n):
    """qr.py::_run builds its Batch with pack=False: a matrix-first view goes down with batch stride 1 and the
    component strides of the view, the two-level batch as n_outer = 3 slabs with the buffer's pitch, both at the
    view's own address; a contiguous batch is one level of back-to-back records (what the register form takes)"""
    from nitorch_fastmath_amd._dispatch import Batch
    from nitorch_fastmath_amd.qr import _dummy
    nb = R.nb_of(n)
    x = torch.arange(nb * n * n, dtype=torch.float64).reshape(nb, n, n)

    def operand(view, ncomp):
        batch = view.shape[:view.dim() - ncomp]
        b = Batch(batch, [view, _dummy(batch, view.dtype, view.device)], [ncomp, 0])
        o = b.operands[0]
        assert b.tensors[0] is view and o.ptr == view.data_ptr()
        return b.n_outer, b.n_inner, o.stride_outer, o.stride_inner, o.stride_row, o.stride_col

    assert operand(R.present(x, 'contiguous'), 2) == (1, nb, 0, n * n, n, 1)
    mf = R.present(x, 'matrix-first')
    assert torch.equal(mf, x) and not mf.is_contiguous()
    assert operand(mf, 2) == (1, nb, 0, 1, n * nb, nb)
    assert operand(R.present(x[:, 0], 'matrix-first'), 1) == (1, nb, 0, 1, 0, nb)
    tl = R.present(x, 'two-level')
    no, pitch, ni = R.TWO_LEVEL
    assert tl.shape == (no, ni, n, n) and torch.equal(tl.reshape(-1, n, n), x[torch.from_numpy(R.two_level_index(nb))])
    assert operand(tl, 2) == (no, ni, pitch * n * n, n * n, n, 1)
    assert operand(R.present(x[:, 0], 'two-level'), 1) == (no, ni, pitch * n, n, 0, 1)
    # the wrap-around of the two-level batch concerns orders 9 and 10 only
    idx = R.two_level_index(nb)
    head = min(nb, 1011)
    assert len(idx) == 1011 and (idx[:head] == np.arange(head)).all() and (idx[head:] == np.arange(1011 - head)).all()


def test_relerr_sees_a_wrong_lane():
    """the batch max-norm the bars use does notice ONE wrong value among a thousand records, and NaN"""
    r = R.records('f32', 9)
    x = r['a'].copy()
    x[517, 3, 4] += 1e-4
    assert relerr(x, r['a']) > 1e-6 and R.worst_record(x, r['a'])[0] == 517
    x[517, 3, 4] = np.nan
    assert not relerr(x, r['a']) <= 1e-6 and not R.same_bits(x, r['a'])
