"""The linear-algebra kernels on hard inputs, one verdict per record (tests/_solver_ref.py has the inputs, the
high-precision truths and the bounds; test_solver_accuracy_host.py shows that the oracle alone passes them):
graded conditioning, exact power-of-two scaling with a different exponent per record, batches that mix positive
definite and failing records at every group and wavefront boundary, barely definite matrices, and one batch
large enough for the second launch.

Every batch is n = 209 (three wavefronts, one full group of 16, one record over) or n = 17, except the last.
No bound is fitted to the kernels: see the module comment of _solver_ref.py.

A inv = I: `batchinv` is held to 4 M . M eps (1 + cond_i / 8).  The oracle's own `sym_invert` (one triangle of a
column-by-column inverse) is up to 5.6 (float32, cond 1e5) and 3.5e6 (float64, cond 1e12) times that: the residual
of a symmetric inverse is of order eps cond^2 for the oracle and the kernels alike, two independent samples of
rounding noise per record (measured: single records of the kernels at 1.2 to 9 times twice the oracle's own, at
every order 5..16).  The symmetric inverses are therefore held to the residual that their forward-error model
implies, |A|_inf max |A^-1| (2 err_oracle,i + M eps (1 + cond_i / 8)), formed from A and the result alone.
"""
import numpy as np
import pytest
import torch
from conftest import EPS
import _solver_ref as R

pytestmark = pytest.mark.gpu
DNS = ['f32', 'f64']
BIG = [M for M in R.ORDERS if M >= 5]


def N():
    import nitorch_fastmath_amd as N_
    return N_


def t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)         # (a copy: the shared inputs are read-only)


def c(x):
    return x.cpu().numpy()


def all_within(excess, n, what):
    """every record of the batch has a verdict and passes: nothing masked, nothing dropped"""
    assert excess.shape == (n,) and not np.isnan(excess).any(), what
    w, i = R.worst(excess)
    assert w <= 1.0, (what, f'record {i}: {w:.3g} times its bound')
    return w


def soa(x):
    """the same values, component-major in memory (a pure SoA / channel-first view)"""
    return x.t().contiguous().t()


# ---------------------------------------------------------------------------------------------- a. graded
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', R.ORDERS)
def test_sym_graded_conditioning_per_record(dev, oracle, dn, M):
    """sym_solve / sym_invert (full, diag) / sym_det on Q diag(lam) Q^T, cond up to 1e5 (float32) / 1e12 (float64).
    M >= 5: backward error of every solve, per-matrix model of every inverse and determinant.  M <= 4: the bits of
    the oracle.

    Measured on an MI355X, worst eta / (M eps) of `sym_solve` over the conds and both batch sizes, float32 / float64
    (the bound is 4 plus twice the oracle's own, which is below 0.1):
      5: 0.13/0.09   6: 0.06/0.06   7: 0.06/0.08   8: 0.10/0.05   9: 0.04/0.05  10: 0.05/0.05
     11: 0.07/0.05  12: 0.04/0.04  13: 0.04/0.04  14: 0.05/0.04  15: 0.04/0.03  16: 0.03/0.03"""
    S = N().sym
    worst = 0.0
    for cond in R.cond_list(M, dn):
        for n in R.NS:
            mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
            md, vd = t(mat, dev), t(vec, dev)
            got = dict(solve=c(S.sym_solve(md, vd)), inv=c(S.sym_invert(md)), diag=c(S.sym_invert(md, diag=True)),
                       det=c(S.sym_det(md)))
            ref = dict(solve=oracle.sym_solve(mat, vec), inv=oracle.sym_invert(mat), diag=oracle.sym_invert(mat, diag=True),
                       det=oracle.sym_det(mat))
            if M <= 4:
                for k in got:
                    assert np.isfinite(ref[k]).all() and R.same_bits(got[k], ref[k]), (k, cond, n)
                continue
            tr = R.sym_truth(mat, dn)
            worst = max(worst, all_within(R.solve_excess(got['solve'], ref['solve'], tr, vec), n, ('solve', cond)))
            eta = R.solve_eta(tr.a, got['solve'], vec, dn).max() / (M * EPS[dn])
            print(f'sym_solve M={M} {dn} cond={cond:g} n={n}: worst eta / (M eps) = {eta:.3f}')
            all_within(R.inv_excess(R.hp_full(got['inv'], dn), R.hp_full(ref['inv'], dn), tr), n, ('invert', cond))
            all_within(R.identity_model_excess(R.hp_full(got['inv'], dn), R.hp_full(ref['inv'], dn), tr), n, ('A inv = I', cond))
            all_within(R.inv_excess(got['diag'], ref['diag'], tr, diag=True), n, ('invert diag', cond))
            all_within(R.det_excess(got['det'], ref['det'], tr), n, ('det', cond))


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', R.ORDERS)
def test_batched_graded_conditioning_per_record(dev, oracle, dn, M):
    """batchinv / batchdet / batchmatvec on U diag(sigma) V^T against the oracle's LU: the per-matrix model, A inv = I
    per record, the matrix-vector product to N eps |A| |v| per component (up to order 4: the bits of the oracle).

    Orders 2 and 3 are adjugate closed forms.  `batchdet` and `batchinv(perturb=True)` are bit-identical to the
    oracle's closed forms at every cond.  The default `batchinv` / `batchdet` of order 2 meet the LU-based bounds
    at every cond (measured up to 1e5 / 1e12: at most 0.35 of them).  Those of ORDER 3 meet them up to cond 1e2
    only and are held to them at cond 1e1, the one cond of this grid below that; measured beyond (worst record,
    inverse and determinant alike / A inv = I, as multiples of the bounds): cond 1e3 1.5 / 0.36, 1e4 6.8 / 1.5,
    1e5 20 / 3.1, 1e6 (float64) 38 / 11, 1e12 1.8e5 / 9.2e4 -- the limit stated in INTEGRATION.md."""
    B = N().batched
    for cond in R.cond_list(M, dn):
        for n in R.NS:
            a, v = R.general_graded(n, M, cond, dn, 200 + M)
            ad = t(a, dev)
            inv, det, mv = c(B.batchinv(ad)), c(B.batchdet(ad)), c(B.batchmatvec(ad, t(v, dev)))
            rinv, rdet, rmv = oracle.batch_inv(a), oracle.batch_det(a), oracle.batch_matvec(a, v)
            assert R.same_bits(mv, rmv) or M > 4
            all_within(R.matvec_excess(mv, a, v, dn), n, ('matvec', cond))
            if M in (2, 3):     # the closed forms that have a counterpart in the oracle: its bits
                rc = oracle.batch_det(a, closed=True)
                assert np.isfinite(rc).all() and R.same_bits(det, rc), (cond, n)
                rc = oracle.batch_inv(a, closed=True)
                assert np.isfinite(rc).all() and R.same_bits(c(B.batchinv(ad, perturb=True)), rc), (cond, n)
            if M == 3 and cond > R.ADJUGATE3_COND_MAX:
                continue
            tr = R.Truth(a, dn)
            all_within(R.inv_excess(inv, rinv, tr), n, ('batchinv', cond))
            all_within(R.det_excess(det, rdet, tr), n, ('batchdet', cond))
            all_within(R.identity_excess(inv, tr), n, ('A inv = I', cond))


# ---------------------------------------------------------------------------------------------- b. scaling
def assert_scaled(got, base, k, what):
    """got == base 2^k per record, bit for bit"""
    want = R.scaled(base, k)
    if not R.same_bits(got, want):
        rows = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(len(got), -1).all(-1))
        raise AssertionError((what, f'{len(rows)} records differ, first {rows[:8]}'))


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', R.ORDERS)
def test_power_of_two_scaling_is_exact_per_record(dev, dn, M):
    """op(2^k_i A_i) is op(A_i) scaled exactly, and sym_solve(A, 2^j_i b_i) = 2^j_i sym_solve(A, b): no tolerance,
    every record with its own exponents.  Contiguous records, in place, and `pivoting='always'`; no eps=.
    An absolute threshold, an overflowing intermediate or a flushed denormal in a kernel would break this; a
    different but scale-covariant rounding cannot.  The exponent ranges (`kmax_for`) keep every expected result a
    normal number (asserted on the CPU)."""
    S, B = N().sym, N().batched
    cond = R.MIXED_COND[dn]
    for n in R.NS:
        mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
        a, v = R.general_graded(n, M, cond, dn, 200 + M)
        km = {op: R.kmax_for(op, M, dn) for op in ('sym_solve', 'sym_invert', 'sym_det', 'batchinv', 'batchdet', 'batchmatvec')}
        ks = {op: R.pow2_scales(n, km[op], 300 + M) for op in km}
        js = {op: R.pow2_scales(n, km[op], 301 + M) for op in km}
        md, vd = t(mat, dev), t(vec, dev)
        for piv in (None, 'always'):
            k, j = ks['sym_solve'], js['sym_solve']
            x = c(S.sym_solve(md, vd, pivoting=piv))
            assert_scaled(c(S.sym_solve(t(R.scaled(mat, k), dev), vd, pivoting=piv)), x, -k, ('sym_solve, matrix', piv))
            assert_scaled(c(S.sym_solve(md, t(R.scaled(vec, j), dev), pivoting=piv)), x, j, ('sym_solve, vector', piv))
            assert_scaled(c(S.sym_solve(t(R.scaled(mat, k), dev), t(R.scaled(vec, j), dev), pivoting=piv)), x, j - k,
                          ('sym_solve, both', piv))
            k = ks['sym_invert']
            ms = t(R.scaled(mat, k), dev)
            assert_scaled(c(S.sym_invert(ms, pivoting=piv)), c(S.sym_invert(md, pivoting=piv)), -k, ('sym_invert', piv))
            assert_scaled(c(S.sym_invert(ms, diag=True, pivoting=piv)), c(S.sym_invert(md, diag=True, pivoting=piv)), -k,
                          ('sym_invert diag', piv))
        # in place
        k, j = ks['sym_solve'], js['sym_solve']
        v2 = t(R.scaled(vec, j), dev)
        S.sym_solve_(t(R.scaled(mat, k), dev), v2)
        assert_scaled(c(v2), c(S.sym_solve(md, vd)), j - k, 'sym_solve_')
        m2 = t(R.scaled(mat, ks['sym_invert']), dev)
        S.sym_invert_(m2)
        assert_scaled(c(m2), c(S.sym_invert(md)), -ks['sym_invert'], 'sym_invert_')
        k = ks['sym_det']
        assert_scaled(c(S.sym_det(t(R.scaled(mat, k), dev))), c(S.sym_det(md)), k * M, 'sym_det')
        ad = t(a, dev)
        k = ks['batchinv']
        assert_scaled(c(B.batchinv(t(R.scaled(a, k), dev))), c(B.batchinv(ad)), -k, 'batchinv')
        k = ks['batchdet']
        assert_scaled(c(B.batchdet(t(R.scaled(a, k), dev))), c(B.batchdet(ad)), k * M, 'batchdet')
        k, j = ks['batchmatvec'], js['batchmatvec']
        assert_scaled(c(B.batchmatvec(t(R.scaled(a, k), dev), t(R.scaled(v, j), dev))), c(B.batchmatvec(ad, t(v, dev))),
                      k + j, 'batchmatvec')


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', [4, 6, 9, 16])
def test_power_of_two_scaling_strided_and_broadcast(dev, dn, M):
    """the same on the pure SoA view and a channel-first field (the strided kernels), and on one Hessian against
    1237 gradients (the broadcast kernels: the one matrix scaled, every gradient with its own exponent)"""
    S = N().sym
    cond = R.MIXED_COND[dn]
    n = 209
    mat, vec = R.spd_graded(n, M, cond, dn, 100 + M)
    k = R.pow2_scales(n, R.kmax_for('sym_solve', M, dn), 300 + M)
    j = R.pow2_scales(n, R.kmax_for('sym_solve', M, dn), 301 + M)
    ki = R.pow2_scales(n, R.kmax_for('sym_invert', M, dn), 300 + M)
    kd = R.pow2_scales(n, R.kmax_for('sym_det', M, dn), 300 + M)
    K = mat.shape[-1]
    views = {'soa': soa,
             'channel-first': lambda x: x.reshape(11, 19, -1).movedim(-1, 0).contiguous().movedim(0, -1)}
    for name, view in views.items():
        md, vd = view(t(mat, dev)), view(t(vec, dev))
        assert not md.is_contiguous()
        x = c(S.sym_solve(md, vd)).reshape(n, M)
        got = S.sym_solve(view(t(R.scaled(mat, k), dev)), view(t(R.scaled(vec, j), dev)))
        assert_scaled(c(got).reshape(n, M), x, j - k, ('sym_solve', name))
        assert_scaled(c(S.sym_invert(view(t(R.scaled(mat, ki), dev)))).reshape(n, K), c(S.sym_invert(md)).reshape(n, K), -ki,
                      ('sym_invert', name))
        assert_scaled(c(S.sym_invert(view(t(R.scaled(mat, ki), dev)), diag=True)).reshape(n, M),
                      c(S.sym_invert(md, diag=True)).reshape(n, M), -ki, ('sym_invert diag', name))
        assert_scaled(c(S.sym_det(view(t(R.scaled(mat, kd), dev)))).reshape(n), c(S.sym_det(md)).reshape(n), kd * M,
                      ('sym_det', name))
        # in place on the strided storage
        v2 = view(t(R.scaled(vec, j), dev))
        S.sym_solve_(view(t(R.scaled(mat, k), dev)), v2)
        assert_scaled(c(v2).reshape(n, M), x, j - k, ('sym_solve_', name))
    # one Hessian, a field of gradients
    nb = 1237
    _, g = R.spd_graded(nb, M, cond, dn, 150 + M)
    jb = R.pow2_scales(nb, R.kmax_for('sym_solve', M, dn), 302 + M)
    one, k1 = mat[:1], int(k[0])
    x = c(S.sym_solve(t(one, dev), t(g, dev)))
    assert x.shape == (nb, M)
    got = c(S.sym_solve(t(R.scaled(one, [k1]), dev), t(R.scaled(g, jb), dev)))
    assert_scaled(got, x, jb - k1, 'one Hessian, many gradients')


# ---------------------------------------------------------------------------------------------- c. mixed batches
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', BIG)
def test_mixed_batches_per_record_scales(dev, oracle, dn, M):
    """positive definite records at cond 1e3 / 1e6 with failing ones at record 0, 15, 16, 63, 64, the first record
    of the ragged last group and the last record, every record times its own power of two: every record, failing
    or not, and every neighbour of a redone group individually.  Out of place and in place.  (Orders 5..8 run the
    pivoted elimination alone.)"""
    S, B = N().sym, N().batched
    for n in R.NS:
        mat, vec, pos = R.mixed_sym(n, M, dn, 400 + M)
        tr = R.sym_truth(mat, dn)
        rs, ri = oracle.sym_solve(mat, vec), R.hp_full(oracle.sym_invert(mat), dn)
        rd = oracle.sym_invert(mat, diag=True)
        md, vd = t(mat, dev), t(vec, dev)
        all_within(R.solve_excess(c(S.sym_solve(md, vd)), rs, tr, vec), n, 'sym_solve')
        gi = R.hp_full(c(S.sym_invert(md)), dn)
        all_within(R.inv_excess(gi, ri, tr), n, 'sym_invert')
        all_within(R.identity_model_excess(gi, ri, tr), n, 'A inv = I')
        all_within(R.inv_excess(c(S.sym_invert(md, diag=True)), rd, tr, diag=True), n, 'sym_invert diag')
        v2, m2 = t(vec, dev), t(mat, dev)
        S.sym_solve_(md, v2)
        S.sym_invert_(m2)
        all_within(R.solve_excess(c(v2), rs, tr, vec), n, 'sym_solve_')
        all_within(R.inv_excess(R.hp_full(c(m2), dn), ri, tr), n, 'sym_invert_')
        all_within(R.identity_model_excess(R.hp_full(c(m2), dn), ri, tr), n, 'A inv = I, in place')
        assert np.array_equal(c(md), mat)                         # the input of the out-of-place calls is untouched
        matd, _, _ = R.mixed_sym(n, M, dn, 400 + M, kmax=R.kmax_for('sym_det', M, dn))
        all_within(R.det_excess(c(S.sym_det(t(matd, dev))), oracle.sym_det(matd), R.sym_truth(matd, dn)), n, 'sym_det')
        for kind in ('reversed', 'late'):
            a, _ = R.mixed_general(n, M, dn, 400 + M, kind)
            tg = R.Truth(a, dn)
            rinv = oracle.batch_inv(a)
            inv = c(B.batchinv(t(a, dev)))
            all_within(R.inv_excess(inv, rinv, tg), n, ('batchinv', kind))
            all_within(R.identity_excess(inv, tg), n, ('A inv = I', kind))
            ad, _ = R.mixed_general(n, M, dn, 400 + M, kind, kmax=R.kmax_for('batchdet', M, dn))
            all_within(R.det_excess(c(B.batchdet(t(ad, dev))), oracle.batch_det(ad), R.Truth(ad, dn)), n, ('batchdet', kind))


# ---------------------------------------------------------------------------------------------- d. barely definite
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('M', BIG)
def test_barely_definite_solves_are_backward_stable(dev, oracle, dn, M):
    """lam_min = c M eps lam_max (c = 0.25, 1, 4, and the two values M^2 below at which the unpivoted attempt
    refuses some records: test_solver_accuracy_host.py counts both kinds): whichever path a record takes, its
    solve meets the backward error bound, which does not depend on cond.  No forward error or determinant is
    asserted here."""
    S = N().sym
    n = 209
    for cc in R.barely_cs(M):
        mat, vec = R.barely_definite(n, M, cc, dn, 500 + M)
        a = R.hp_full(mat, dn)
        md, vd = t(mat, dev), t(vec, dev)
        ref = R.solve_eta(a, oracle.sym_solve(mat, vec), vec, dn)
        for got in (c(S.sym_solve(md, vd)), c(S.sym_solve(soa(md), soa(vd)))):
            eta = R.solve_eta(a, got, vec, dn)
            all_within(eta / R.eta_bound(ref, M, dn), n, ('sym_solve', cc))


# ---------------------------------------------------------------------------------------------- e. second launch
def test_second_launch_redoes_marked_groups_and_nothing_else(dev, oracle):
    """M = 9, float32, n = 2^20 + 1, per-record scales, a failing record every 4099 and at both ends: sym_solve
    and batchinv per record on both ends of the batch, the marked groups and their neighbours; and every selected
    group that was NOT marked is bit-identical to the same records solved in a batch of 209 (the mark and redo
    pass changed nothing it should not)."""
    S, B = N().sym, N().batched
    M, dn = 9, 'f32'
    n, bad, sel = R.BIG_N, R.big_fail_positions(), R.big_selection()
    k = R.pow2_scales(n, R.KMAX_LINEAR[dn], 77)
    base, vbase = R.spd_graded(R.BIG_BASE, M, R.MIXED_COND[dn], dn, 600)
    marked = np.isin(sel // 16, np.unique(bad // 16))
    clean = sel[~marked]
    clean = clean[: len(clean) // 209 * 209]
    assert len(clean) >= 209 and marked.sum() >= 40 * 16

    # compact symmetric
    mat = R.big_tile(base, k)
    vec = vbase[np.arange(n) % R.BIG_BASE]
    mat[bad] = R.scaled(R.indefinite(len(bad), M, dn, 601), k[bad])
    got = c(S.sym_solve(t(mat, dev), t(vec, dev))[torch.from_numpy(sel).to(dev)])
    ms, vs = mat[sel], vec[sel]
    all_within(R.solve_excess(got, oracle.sym_solve(ms, vs), R.sym_truth(ms, dn), vs), len(sel), 'sym_solve')
    assert (R.ldl_pivots(ms[~marked], dn) > 0).all()          # no unmarked group holds a record the first launch refuses
    small = np.concatenate([c(S.sym_solve(t(mat[q], dev), t(vec[q], dev))) for q in clean.reshape(-1, 209)])
    assert np.array_equal(got[~marked][: len(small)], small)
    del mat, vec

    # general
    a = R.to_full(base).astype(np.float32)
    odd = (np.random.default_rng(602).standard_normal((len(bad), M, M)) * 0.1 + np.eye(M))[:, ::-1].astype(np.float32)
    ad = t(a, dev)[torch.from_numpy(np.arange(n) % R.BIG_BASE).to(dev)]
    kd = torch.from_numpy(np.array(k)).to(dev)
    ad = torch.ldexp(ad, kd[:, None, None].to(torch.int32))
    ad[torch.from_numpy(bad).to(dev)] = t(R.scaled(odd, k[bad]), dev)
    asel = c(ad[torch.from_numpy(sel).to(dev)])
    inv = c(B.batchinv(ad)[torch.from_numpy(sel).to(dev)])
    tg = R.Truth(asel, dn)
    all_within(R.inv_excess(inv, oracle.batch_inv(asel), tg), len(sel), 'batchinv')
    all_within(R.identity_excess(inv, tg), len(sel), 'A inv = I')
    assert R.diagonal_pivots_ok(asel[~marked]).all()
    idx = torch.from_numpy(clean).to(dev)
    small = np.concatenate([c(B.batchinv(ad[idx[q:q + 209]].contiguous())) for q in range(0, len(clean), 209)])
    assert np.array_equal(inv[~marked][: len(small)], small)


# ---------------------------------------------------------------------------------------------- f. fused
@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('kd', [(3, 3), (6, 6), (9, 9)])
def test_matmul_solve_on_graded_hessians_equals_the_chain(dev, dn, kd):
    """`sym_matmul_solve` is bit-identical to sym_solve(sym_matmul(j, h), g) (the relation of
    test_gpu_sym.py::test_fused_matmul_solve_equals_the_chain), here per record on graded Hessians with a power
    of two of their own"""
    S = N().sym
    k_, d = kd
    for n in R.NS:
        h, g = R.spd_graded(n, k_, R.MIXED_COND[dn], dn, 700 + k_)
        h = R.scaled(h, R.pow2_scales(n, R.KM_MAX[dn] // (k_ + 1) // 2, 701))
        # orthogonal jacobians (times 2): J^T H J keeps the cond of H, at which the closed forms of k = 3 are finite
        j = (2 * np.linalg.qr(np.random.default_rng(702 + n).standard_normal((n, k_, d)))[0]).astype(R.NP[dn])
        jd, hd, gd = t(j, dev), t(h, dev), t(g, dev)
        fused, chain = c(S.sym_matmul_solve(jd, hd, gd)), c(S.sym_solve(S.sym_matmul(jd, hd), gd))
        same = ((fused == chain) | (np.isnan(fused) & np.isnan(chain))).all(-1)
        assert same.shape == (n,) and same.all(), np.flatnonzero(~same)[:8]
        assert np.isfinite(chain).all() and R.is_normal(h, dn)
