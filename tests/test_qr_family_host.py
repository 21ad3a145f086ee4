"""The ORACLE's QR building blocks held to the per-record bounds of tests/_qr_ref.py at orders 1..8, both dtypes,
on every family -- no exclusion list.  The kernels run the oracle's operation order (test_gpu_qr_family.py asserts
bit identity), so what the oracle gets wrong the kernels get wrong with it: this file is where an arithmetic
fault of the family shows without a GPU.  Before the range guard of the building blocks it
failed on the `tiny rows` and `tiny border` cells, the 2^-70 / 2^-525 vectors and pairs and a few cells of rank-one records;
profiles/qr_family_accuracy.md has both sets of ratios.

Every test prints its `qr-family` lines (worst ratio per operation and family) before it asserts anything."""
import numpy as np
import pytest
from conftest import relerr
import _qr_ref as R


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.ORDERS)
def test_oracle_within_bounds(oracle, dn, n):
    w = R.worst(dn, n, R.score(dn, n, R.oracle_results(oracle, dn, n)))
    R.report('oracle', dn, n, w)
    assert not R.exceeding(w), R.exceeding(w)


def test_batch_is_what_the_judges_assume():
    """the batch shape, the exactness of the integer families and the +0 zeros the bit-for-bit demands rely on"""
    assert R.NB == 1200 and R.NB % 64 != 0 and R.NB > 2 * 512
    for dn in ('f32', 'f64'):
        for n in R.ORDERS:
            a, cells = R.matrices(dn, n)
            assert sorted(np.concatenate(list(cells.values()))) == list(range(R.NB))
            assert np.isfinite(a).all() and not np.signbit(a[a == 0]).any()
            for fam in ('integer rank 1', 'integer rank 2'):
                assert np.array_equal(a[cells[fam]], np.round(a[cells[fam]]))
            if n >= 3:
                assert np.linalg.matrix_rank(a[cells['integer rank 1']].astype(np.float64)).max() <= 1
                assert np.linalg.matrix_rank(a[cells['integer rank 2']].astype(np.float64)).max() <= 2
                s = R.TINY_SHIFTS[dn][-1]
                t = a[cells[f'tiny rows 2^-{s}']]
                assert np.abs(t[:, 2:]).max() < 2.0 ** (3 - s) and np.abs(t[:, :2]).max() > 0.5
                assert (t[:, 2:] != 0).all()


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_judges_notice_a_small_wrong_record(oracle, dn):
    """one record 2^-60 of its neighbours' size, entirely wrong: invisible to conftest.relerr, far above 1 for
    the per-record judges (the pattern of test_eig_sym_accuracy_host.py)"""
    n = 4
    recs, cells = R.matrices(dn, n)
    a = recs[np.concatenate([cells['normal'], cells['graded cols'][:1]])].copy()       # 64 records and the small one
    a[64] = np.ldexp(a[64], -60)
    h, us = oracle.hessenberg(a, True)
    hz = np.triu(a, -1)
    q, r = oracle.qr_hessenberg(hz)
    good_h = R._similarity(dn, n, a, h, us)
    good_q = R.judge_qr_hessenberg(dn, n, hz, q, r)['Q R = H']
    assert good_h.max() <= R.C and good_q.max() <= R.C
    h_bad, r_bad = h.copy(), r.copy()
    h_bad[64] = h[64, ::-1, ::-1].T          # another matrix of the same size
    r_bad[64] = 2 * r[64]
    assert relerr(h_bad, h) <= 1e-15 and relerr(r_bad, r) <= 1e-15
    assert R._similarity(dn, n, a, h_bad, us)[64] > 1e3 * R.C
    assert R.judge_qr_hessenberg(dn, n, hz, q, r_bad)['Q R = H'][64] > 1e3 * R.C
    assert R._similarity(dn, n, a, h_bad, us)[:64].max() <= R.C


def test_judges_notice_each_fault():
    """every metric of the judges moves when the property it guards is broken (float64, n = 5, normal records)"""
    dn, n = 'f64', 5
    rng = np.random.default_rng(5)
    x = rng.standard_normal((8, n))
    nx = np.sqrt((x * x).sum(-1))
    alpha = -np.sign(x[:, 0]) * nx
    v = x.copy()
    v[:, 0] -= alpha
    u = v / np.sqrt((v * v).sum(-1, keepdims=True))
    ok = R.judge_householder(dn, n, 0, x, u, alpha)
    assert max(s.max() for s in ok.values()) <= 2.0
    assert R.judge_householder(dn, n, 0, x, u * (1 - 4e-4), alpha)['unit'].min() > 1e9     # |u| = 0.9996
    assert R.judge_householder(dn, n, 0, x, u * (1 - 4e-4), alpha)['reflects'].min() > 1e9
    assert np.isinf(R.judge_householder(dn, n, 0, x, u, -alpha)['sign']).all()
    assert R.judge_householder(dn, n, 0, x, u, alpha * (1 + 1e-9))['alpha'].min() > 1e5
    z = np.zeros((8, n))
    assert np.isinf(R.judge_householder(dn, n, 0, z, z + 1e-300, z[:, 0])['zero exact']).all()
    assert np.isinf(R.judge_householder(dn, n, 0, x, u * np.nan, alpha)['unit']).all()
    c, s = x[:, 0] / np.hypot(x[:, 0], x[:, 1]), -x[:, 1] / np.hypot(x[:, 0], x[:, 1])
    assert max(v.max() for v in R.judge_givens(dn, x[:, 0], x[:, 1], c, s).values()) <= 2.0
    assert R.judge_givens(dn, x[:, 0], x[:, 1], c * (1 - 4e-4), s)['unit'].max() > 1e9
    assert R.judge_givens(dn, x[:, 0], x[:, 1], c, -s)['annihilates'].min() > 1e9
    assert R.judge_givens(dn, x[:, 0], x[:, 1], -c, -s)['r'].min() > 1e9
    assert np.isinf(R.judge_givens(dn, x[:, 0], 0 * x[:, 1], np.sign(x[:, 0]) * (1 - 1e-16), 0 * s)['axis exact']).all()
    # dense products: a rotation and a reflection applied by hand
    a = rng.standard_normal((8, n, n))
    cc, ss = c[:, None], s[:, None]
    want = a.copy()
    want[:, 0], want[:, n - 1] = a[:, 0] * cc - ss * a[:, n - 1], a[:, n - 1] * cc + ss * a[:, 0]
    # (the first N_IDENTITY records of a batch are the bit-for-bit ones: here that is all eight)
    assert R.judge_givens_apply(dn, n, a, cc, ss, 0, n - 1, 'left', want)['product'].max() <= 2.0
    assert R.judge_givens_apply(dn, n, a, cc, ss, n - 1, 0, 'left', want)['product'].min() > 1e9   # the other orientation
    assert R.judge_givens_apply(dn, n, a, cc, ss, 0, n - 1, 'right', want)['product'].min() > 1e9
    one, nil = np.ones((8, 1)), np.zeros((8, 1))
    assert R.judge_givens_apply(dn, n, a, one, nil, 0, n - 1, 'both', a)['(1, 0) exact'].max() == 0
    moved = a.copy()
    moved[0, 0, 0] = np.nextafter(a[0, 0, 0], 9.0)
    assert np.isinf(R.judge_givens_apply(dn, n, a, one, nil, 0, n - 1, 'both', moved)['(1, 0) exact'][0])
    got = a - 2 * np.einsum('bi,bj,bjk->bik', u, u, a)
    assert R.judge_householder_apply(dn, n, a, [u], 'left', False, got)['product'].max() <= 2.0
    assert R.judge_householder_apply(dn, n, a, [u], 'right', False, got)['product'].min() > 1e9
    assert np.isinf(R.judge_householder_apply(dn, n, a, [0 * u], 'left', False, moved)['u = 0 exact'][0])
    # structure: one entry below the subdiagonal, the wrong triangle
    am = R.matrices(dn, n)[0][R.matrices(dn, n)[1]['normal'][:8]]                      # general: the triangles differ
    cells = {'zero': np.arange(0), 'diagonal': np.arange(0)}
    h = np.triu(am, -1)
    e = [np.zeros((8, n - 1 - k)) for k in range(n - 2)]
    assert R.judge_hessenberg(dn, n, am, h, h, e, cells)['structure'].max() == 0
    h2 = h.copy()
    h2[3, n - 1, 0] = 1e-300
    assert np.isinf(R.judge_hessenberg(dn, n, am, h2, h2, e, cells)['structure'][3])
    assert np.isinf(R.judge_hessenberg(dn, n, am, h, h2, e, cells)['same without u'][3])
    assert R._similarity(dn, n, R.sym_read(am, True), R.sym_read(am, True), e).max() == 0
    assert R._similarity(dn, n, R.sym_read(am, True), R.sym_read(am, False), e).min() > 1e9


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.LARGE_ORDERS)
def test_oracle_tiny_rows_large_orders(oracle, dn, n):
    """the `tiny rows` and `tiny border` families through every guarded operation at orders 9, 12 and 16"""
    w = R.worst_tiny(dn, n, R.run_tiny(oracle, dn, n))
    R.report('oracle', dn, n, w)
    assert not R.exceeding(w), R.exceeding(w)
