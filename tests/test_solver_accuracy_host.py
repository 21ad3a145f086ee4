"""The inputs, truths and bounds of tests/_solver_ref.py, run against the CPU oracle: the reference alone passes
every bound that test_gpu_solver_accuracy.py imposes on the kernels (its floors alone, without the 2 err_oracle
term), on 100 % of the records of every family, and the generated inputs have the properties the GPU tests rely
on (no GPU needed).  `pytest -s` prints the oracle's worst ratios per family.

Measured here (oracle, worst record of n = 209 and 17 over every order 5..16 and every cond of the family):
  sym_solve   eta / (M eps)                  0.092 (f32), 0.093 (f64)   spd_graded
  sym_solve   eta / (M eps)                  0.077 (f32), 0.073 (f64)   barely_definite
  sym_invert  err / (M eps (1 + cond / 8))   0.209 (f32), 0.204 (f64)   (full and diag)
  sym_det     err / (M eps (1 + cond / 8))   0.287 (f32), 0.276 (f64)
  sym_invert  |A inv - I| / bound            5.6   (f32), 3.5e6 (f64)   NOT met by the oracle: one triangle of a
                                             column-by-column inverse; asserted for batchinv only, where it holds
  batchinv / batchdet / batchmatvec          all below 1, printed per order
"""
import numpy as np
import pytest
from conftest import EPS
import _solver_ref as R

DNS = ['f32', 'f64']
BIG = [M for M in R.ORDERS if M >= 5]


def every_record(ratio, n):
    """a per-record ratio covers the whole batch and is a number everywhere: nothing masked, nothing dropped"""
    assert ratio.shape == (n,) and not np.isnan(ratio).any()
    return float(ratio.max())


def exact_inv_det(a):
    """inverse and determinant of one float64 matrix in exact rational arithmetic (Gauss-Jordan on Fractions)"""
    from fractions import Fraction
    N = len(a)
    m = [[Fraction(float(v)) for v in row] + [Fraction(int(i == j)) for j in range(N)] for i, row in enumerate(a)]
    det = Fraction(1)
    for k in range(N):
        p = max(range(k, N), key=lambda r: abs(m[r][k]))
        if p != k:
            m[k], m[p] = m[p], m[k]
            det = -det
        det *= m[k][k]
        m[k] = [v / m[k][k] for v in m[k]]
        for r in range(N):
            if r != k and m[r][k] != 0:
                f = m[r][k]
                m[r] = [x - f * y for x, y in zip(m[r], m[k])]
    return [row[N:] for row in m], det


@pytest.mark.parametrize('dn,M', [('f64', 16), ('f64', 9), ('f64', 5), ('f32', 16)])
def test_high_precision_truth_is_within_a_sixteenth_of_the_bounds(dn, M):
    """the truths at the highest cond of the dtype, where the requirement bites, against exact rational
    arithmetic: the inverse, the determinant and cond_inf of `Truth` on records of both graded families, and
    a residual computed in high precision against the exact one"""
    from fractions import Fraction
    assert R.hp_ok()
    cond = R.CONDS[dn][-1]
    mat, vec = R.spd_graded(17, M, cond, dn, 100 + M)
    a, _ = R.general_graded(17, M, cond, dn, 200 + M)
    for full in (R.to_full(mat)[:2], a[:2].astype(np.float64)):
        tr = R.Truth(full, dn)
        for i in range(len(full)):
            inv, det = exact_inv_det(full[i])
            big = max(abs(v) for row in inv for v in row)
            err = max(abs(Fraction(float(tr.inv[i, r, q])) - inv[r][q]) for r in range(M) for q in range(M)) / big
            floor = R.model_floor(M, dn, tr.cond[i])
            assert float(err) <= floor / 16, (float(err), floor)
            # (float() of the high-precision value: 2^-53 more, far below floor / 16)
            d = Fraction(float(tr.det[i])) * Fraction(2) ** int(tr.dexp[i])
            assert float(abs(d / det - 1)) <= floor / 16
            ci = max(sum(abs(v) for v in row) for row in inv) * Fraction(float(np.abs(full[i]).sum(-1).max()))
            assert abs(tr.cond[i] / float(ci) - 1) <= 1e-3
            # residual of a rounded solution: high precision against exact
            x = np.linalg.solve(full[i], vec[i].astype(np.float64)).astype(R.NP[dn])
            eta = R.solve_eta(tr.a[i:i + 1], x[None], vec[i:i + 1], dn)[0]
            r = max(abs(Fraction(float(vec[i, p])) - sum(Fraction(float(full[i, p, q])) * Fraction(float(x[q])) for q in range(M)))
                    for p in range(M))
            den = Fraction(float(np.abs(full[i]).sum(-1).max())) * max(abs(Fraction(float(v))) for v in x) + \
                max(abs(Fraction(float(v))) for v in vec[i])
            assert abs(eta - float(r / den)) <= 4 * M * EPS[dn] / 16


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', R.ORDERS)
def test_graded_inputs_have_their_properties(dn, M):
    for cond in R.CONDS[dn]:
        for n in R.NS:
            mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
            assert mat.dtype == R.NP[dn] and mat.shape == (n, M * (M + 1) // 2) and vec.shape == (n, M)
            full = R.to_full(mat)
            c2 = np.linalg.cond(full)
            nominal = cond if M > 1 else 1.0
            assert (c2 <= 2 * nominal).all() and (c2 >= nominal / 2).all(), (cond, c2.min(), c2.max())
            # still positive definite after the rounding: every pivot of the float64 factorisation positive
            assert (R.ldl_pivots(mat, 'f64') > 0).all()
            a, _ = R.general_graded(n, M, cond, dn, 200 + M)
            c2 = np.linalg.cond(a.astype(np.float64))
            assert (c2 <= 2 * nominal).all() and (c2 >= nominal / 2).all(), (cond, c2.min(), c2.max())
    with pytest.raises(ValueError):
        R.spd_graded(17, max(M, 2), 1.0 / EPS[dn], dn, 1)
    k = R.pow2_scales(209, 40, 5)
    assert k.min() == -40 and k.max() == 40 and len(np.unique(k)) > 60
    assert np.array_equal(R.scaled(mat, R.pow2_scales(len(mat), 3, 1)).astype(np.float64) /
                          np.ldexp(1.0, R.pow2_scales(len(mat), 3, 1))[:, None], mat.astype(np.float64))


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', BIG)
def test_oracle_sym_within_the_floors_on_graded_input(oracle, dn, M):
    w = dict(eta=0.0, inv=0.0, invdiag=0.0, det=0.0, eye=0.0)
    for cond in R.CONDS[dn]:
        for n in R.NS:
            mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
            tr = R.sym_truth(mat, dn)
            assert (tr.cond >= 1).all() and (tr.cond <= 2 * M * cond).all()
            eta = R.solve_eta(tr.a, oracle.sym_solve(mat, vec), vec, dn)
            w['eta'] = max(w['eta'], every_record(eta / (M * EPS[dn]), n))
            assert (eta <= 4 * M * EPS[dn]).all()
            inv = R.hp_full(oracle.sym_invert(mat), dn)
            floor = R.model_floor(M, dn, tr.cond)
            w['inv'] = max(w['inv'], every_record(R.inv_err(inv, tr.inv, dn) / floor, n))
            dg = np.diagonal(tr.inv, axis1=1, axis2=2)
            w['invdiag'] = max(w['invdiag'], every_record(R.inv_err(oracle.sym_invert(mat, diag=True), dg, dn) / floor, n))
            w['det'] = max(w['det'], every_record(R.det_err(oracle.sym_det(mat), tr.det, tr.dexp, dn) / floor, n))
            w['eye'] = max(w['eye'], every_record(R.identity_excess(inv, tr), n))
            assert every_record(R.identity_model_excess(inv, inv, tr), n) <= 1.0
    print(f'oracle sym M={M} {dn}: eta/(M eps) {w["eta"]:.3f}; err/floor inv {w["inv"]:.3f} diag {w["invdiag"]:.3f} '
          f'det {w["det"]:.3f}; |A inv - I|/bound {w["eye"]:.4f}')
    assert max(w['inv'], w['invdiag'], w['det']) <= 1.0
    assert np.isfinite(w['eye'])      # (printed: the oracle is beyond the plain bound here; see identity_model_excess)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('N', BIG)
def test_oracle_batched_within_the_floors_on_graded_input(oracle, dn, N):
    w = dict(inv=0.0, det=0.0, eye=0.0, mv=0.0)
    for cond in R.CONDS[dn]:
        for n in R.NS:
            a, v = R.general_graded(n, N, cond, dn, 200 + N)
            tr = R.Truth(a, dn)
            floor = R.model_floor(N, dn, tr.cond)
            inv = oracle.batch_inv(a)
            w['inv'] = max(w['inv'], every_record(R.inv_err(inv, tr.inv, dn) / floor, n))
            w['det'] = max(w['det'], every_record(R.det_err(oracle.batch_det(a), tr.det, tr.dexp, dn) / floor, n))
            w['eye'] = max(w['eye'], every_record(R.identity_excess(inv, tr), n))
            w['mv'] = max(w['mv'], every_record(R.matvec_excess(oracle.batch_matvec(a, v), a, v, dn), n))
    print(f'oracle batched N={N} {dn}: err/floor inv {w["inv"]:.3f} det {w["det"]:.3f}; |A inv - I|/bound {w["eye"]:.4f}; '
          f'matvec/(N eps |A||v|) {w["mv"]:.3f}')
    assert max(w.values()) <= 1.0


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', [1, 2, 3, 4])
def test_oracle_closed_forms_are_finite_up_to_their_cond(oracle, dn, M):
    """orders 1..4 are held to bit equality with the oracle, which needs a finite oracle to mean something"""
    assert R.cond_list(M, dn) == tuple(c for c in R.CONDS[dn] if c <= R.CLOSED_COND_MAX[dn]) and len(R.cond_list(M, dn)) == 2
    for cond in R.cond_list(M, dn):
        for n in R.NS:
            mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
            a, v = R.general_graded(n, M, cond, dn, 200 + M)
            for r in (oracle.sym_solve(mat, vec), oracle.sym_invert(mat), oracle.sym_invert(mat, diag=True),
                      oracle.sym_det(mat), oracle.batch_inv(a), oracle.batch_det(a), oracle.batch_matvec(a, v)):
                assert len(r) == n and np.isfinite(r).all()


def scale_cases(M, dn):
    """(op name, kmax) of every op of the scaling tests at this order"""
    return [(op, R.kmax_for(op, M, dn)) for op in ('sym_solve', 'sym_invert', 'sym_det', 'batchinv', 'batchdet', 'batchmatvec')]


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', R.ORDERS)
def test_oracle_scales_exactly_and_the_scaled_results_are_normal(oracle, dn, M):
    """op(2^k_i A_i) is the exactly scaled op(A_i), bit for bit, for the oracle; and the expected scaled results
    are normal numbers of the dtype, so that the same assertion on the kernels is one about their arithmetic
    and not about the ends of the number format"""
    cond = R.MIXED_COND[dn]
    for n in R.NS:
        mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
        a, v = R.general_graded(n, M, cond, dn, 200 + M)
        for op, kmax in scale_cases(M, dn):
            assert kmax >= 1
            k = R.pow2_scales(n, kmax, 300 + M)
            if op == 'sym_solve':
                j = R.pow2_scales(n, kmax, 301 + M)          # the right-hand sides' own powers of two
                want = R.scaled(oracle.sym_solve(mat, vec), j - k)
                got = oracle.sym_solve(R.scaled(mat, k), R.scaled(vec, j))
            elif op == 'sym_invert':
                want, got = R.scaled(oracle.sym_invert(mat), -k), oracle.sym_invert(R.scaled(mat, k))
                assert R.same_bits(oracle.sym_invert(R.scaled(mat, k), diag=True), R.scaled(oracle.sym_invert(mat, diag=True), -k))
            elif op == 'sym_det':
                want, got = R.scaled(oracle.sym_det(mat), k * M), oracle.sym_det(R.scaled(mat, k))
            elif op == 'batchinv':
                want, got = R.scaled(oracle.batch_inv(a), -k), oracle.batch_inv(R.scaled(a, k))
            elif op == 'batchdet':
                want, got = R.scaled(oracle.batch_det(a), k * M), oracle.batch_det(R.scaled(a, k))
            else:
                j = R.pow2_scales(n, kmax, 301 + M)
                want, got = R.scaled(oracle.batch_matvec(a, v), k + j), oracle.batch_matvec(R.scaled(a, k), R.scaled(v, j))
            assert want.shape[0] == n and R.is_normal(want, dn), (op, kmax)        # every entry: no zeros either
            assert R.same_bits(got, want), (op, n, kmax)


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', BIG)
def test_mixed_batches_fail_where_they_should_and_the_oracle_passes(oracle, dn, M):
    for n in R.NS:
        pos = np.array(R.fail_positions(n))
        assert {0, 15, 16, n - 1} <= set(pos) and (n < 65 or {63, 64, (n - 1) // 16 * 16} <= set(pos))
        bad = np.zeros(n, bool)
        bad[pos] = True
        mat, vec, p = R.mixed_sym(n, M, dn, 400 + M)
        assert np.array_equal(p, pos)
        # what the unpivoted first attempt sees: a non-positive pivot exactly at the placed records
        assert np.array_equal((R.ldl_pivots(mat, dn) > 0).all(-1), ~bad)
        tr = R.sym_truth(mat, dn)
        e = np.log2(np.abs(tr.a).reshape(n, -1).max(-1).astype(np.float64))
        assert e.max() - e.min() > R.KMAX_LINEAR[dn]                # per-record scales: a batch max-norm sees one record
        eta = R.solve_eta(tr.a, oracle.sym_solve(mat, vec), vec, dn)
        assert every_record(eta / (4 * M * EPS[dn]), n) <= 1.0
        floor = R.model_floor(M, dn, tr.cond)
        assert every_record(R.inv_err(R.hp_full(oracle.sym_invert(mat), dn), tr.inv, dn) / floor, n) <= 1.0
        matd, _, _ = R.mixed_sym(n, M, dn, 400 + M, kmax=R.kmax_for('sym_det', M, dn))
        trd = R.sym_truth(matd, dn)
        ref = oracle.sym_det(matd)
        assert R.is_normal(ref, dn)
        assert every_record(R.det_err(ref, trd.det, trd.dexp, dn) / R.model_floor(M, dn, trd.cond), n) <= 1.0
        for kind in ('reversed', 'late'):
            a, p = R.mixed_general(n, M, dn, 400 + M, kind)
            assert np.array_equal(p, pos)
            if M >= 9:      # the diagonal-first attempt of orders 9..16: refused at every placed record; a few of the
                ok = R.diagonal_pivots_ok(a)     # others are refused too (their groups then take the pivoted path as well),
                assert not ok[pos].any()         # but whole groups remain that the pivoted path never touches
                clean = [g for g in range(n // 16) if ok[16 * g:16 * g + 16].all()]
                assert n < 64 or len(clean) >= 3, (kind, clean)
            tg = R.Truth(a, dn)
            assert every_record(R.inv_err(oracle.batch_inv(a), tg.inv, dn) / R.model_floor(M, dn, tg.cond), n) <= 1.0
            ad, _ = R.mixed_general(n, M, dn, 400 + M, kind, kmax=R.kmax_for('batchdet', M, dn))
            tgd = R.Truth(ad, dn)
            ref = oracle.batch_det(ad)
            assert R.is_normal(ref, dn)
            assert every_record(R.det_err(ref, tgd.det, tgd.dexp, dn) / R.model_floor(M, dn, tgd.cond), n) <= 1.0


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', BIG)
def test_barely_definite_has_both_kinds_and_the_oracle_solves_it(oracle, dn, M):
    """lam_min = c M eps lam_max: the unpivoted factorisation in the dtype ends on a tiny positive pivot for some
    records and on a negative one for others; the solve's backward error does not depend on cond"""
    kinds = np.zeros(2, int)
    worst = 0.0
    for c in R.barely_cs(M):
        mat, vec = R.barely_definite(209, M, c, dn, 500 + M)
        assert (np.linalg.eigvalsh(np.asarray(R.hp_full(mat, dn), np.float64)).max(-1) > 0.5).all()
        ok = (R.ldl_pivots(mat, dn) > 0).all(-1)
        kinds += (int(ok.sum()), int((~ok).sum()))
        tr_a = R.hp_full(mat, dn)
        eta = R.solve_eta(tr_a, oracle.sym_solve(mat, vec), vec, dn)
        worst = max(worst, every_record(eta / (M * EPS[dn]), 209))
        assert (eta <= 4 * M * EPS[dn]).all()
    print(f'barely definite M={M} {dn}: {kinds[0]} records pass the unpivoted attempt, {kinds[1]} do not; '
          f'oracle eta/(M eps) {worst:.3f}')
    assert kinds.min() >= 16


def test_second_launch_selection_covers_marked_groups_and_clean_ones():
    bad, sel = R.big_fail_positions(), R.big_selection()
    assert R.BIG_N == (1 << 20) + 1 and bad[0] == 0 and bad[-1] == R.BIG_N - 1 and (np.diff(bad)[:-1] == R.BIG_EVERY).all()
    marked = np.unique(bad // 16)
    sel_groups = np.unique(sel // 16)
    assert np.isin(marked[:40], sel_groups).all() and np.isin(marked[-2:], sel_groups).all()
    clean = np.setdiff1d(sel_groups, marked)
    assert len(clean) > 2 * 40                                        # neighbours on both sides
    assert {0, R.BIG_N - 1} <= set(sel) and len(sel) < 4000
