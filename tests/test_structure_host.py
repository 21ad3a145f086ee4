"""The references and bounds of tests/_dense_ref.py, run against the CPU oracle on the seeded inputs of
test_gpu_sym_structure.py / test_gpu_autograd_shapes.py: the reference alone passes every bound that the
GPU tests impose on the kernels (no GPU needed)."""
import numpy as np
import pytest
from conftest import TOL, relerr
import _dense_ref as R


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', R.ORDERS)
def test_compact_full_round_trip(oracle, dn, M):
    mat, _ = R.spd_np(65, M, R.NP[dn], 40 + M)
    full = R.to_full(mat)
    assert full.shape == (65, M, M) and np.array_equal(full, full.transpose(0, 2, 1))
    assert np.array_equal(full, oracle.sym_to_full(mat).astype(np.float64))
    assert np.array_equal(R.to_compact(full), mat.astype(np.float64))
    assert [full[0, i, j] for i, j in R.pairs(M)] == list(mat[0].astype(np.float64))
    assert R.order_of(mat.shape[-1]) == M


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('diag', [False, True], ids=['sym', 'diag'])
@pytest.mark.parametrize('n', [65, 1573])
@pytest.mark.parametrize('k', R.KD)
def test_oracle_matmul_within_the_derived_bound(oracle, dn, diag, n, k):
    worst = 0.0
    for d in R.KD:
        j, h = R.matmul_inputs(n, k, d, dn, diag)
        ref = oracle.sym_matmul(j, h)
        truth, S, T = R.matmul_truth(j, h)
        assert T == (k if (diag and k != 1) else k * (k + 1) // 2)
        assert ref.shape == truth.shape == (n, d * (d + 1) // 2)
        ex = R.matmul_excess(ref, j, h, dn)
        worst = max(worst, ex * (T + 4))
        assert ex <= 1.0, (k, d, ex)
        assert relerr(ref, truth) <= TOL[dn], (k, d)
    print(f'worst |oracle - truth| / (eps S) at k={k}: {worst:.2f}')


def test_matmul_truth_knows_the_transposed_cases():
    """quirk Q16 is in the truth where the oracle has it, and only there"""
    rng = np.random.default_rng(3)
    for k, d in ((2, 2), (3, 3), (4, 4), (2, 3)):
        j = rng.standard_normal((5, k, d))
        h, _ = R.spd_np(5, k, np.float64, 11)
        jt = np.swapaxes(j, -1, -2)
        plain = R.to_compact(jt @ R.to_full(h) @ j)
        truth = R.matmul_truth(j, h)[0]
        if R.matmul_flips(k, d, False):
            assert np.allclose(truth, R.to_compact(j @ R.to_full(h) @ jt)) and not np.allclose(truth, plain)
        else:
            assert np.allclose(truth, plain)
        hd = np.ascontiguousarray(h[:, :k])
        jd = np.einsum('nkd,nk,nke->nde', j, hd, j)
        assert np.allclose(R.matmul_truth(j, hd)[0], R.to_compact(jd))


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('M', R.ORDERS)
def test_outer2_formula_within_the_derived_bound(oracle, dn, M):
    for n in R.NS:
        x, y = R.outer2_inputs(n, M, dn)
        got = R.outer2_formula(x, y)
        assert got.dtype == R.NP[dn] and got.shape == (n, M * (M + 1) // 2)
        assert R.outer2_excess(got, x, y, dn) <= 1.0
        assert R.outer2_excess(R.outer2_formula(x, y, True), x, y, dn, neg=True) <= 1.0
        # x = y: twice the off-diagonals of the symmetric outer product, exactly
        o = oracle.sym_outer(x)
        o[:, M:] *= 2
        assert np.array_equal(R.outer2_formula(x, x), o)
    # the truth is the pull-back of u v^T onto compact storage: <outer2(u, v), c> = u^T full(c) v
    u, v = R.outer2_inputs(63, M, 'f64')
    c, _ = R.spd_np(63, M, np.float64, 5)
    lhs = (R.outer2_truth(u, v)[0] * c).sum(-1)
    rhs = np.einsum('ni,nij,nj->n', u, R.to_full(c), v)
    assert np.allclose(lhs, rhs, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('n', [2, 3, 4, 6])
def test_eig_inputs_keep_their_gap(n):
    a, lam = R.eig_inputs(197, n, 600 + n)
    assert a.shape == (197, n, n) and np.array_equal(a, a.transpose(0, 2, 1))
    assert np.diff(lam, axis=-1).min() >= R.EIG_GAP
    assert np.allclose(np.linalg.eigvalsh(a), lam, rtol=0, atol=1e-12)
    assert R.eig_gap(a) >= R.EIG_GAP * (1 - 1e-9)
    assert R.eig_gap(a.astype(np.float32)) >= R.EIG_GAP * (1 - 1e-5)     # what the float32 tests run on
