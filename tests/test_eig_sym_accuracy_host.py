"""The CPU oracle's eig_sym held to the per-record bars of tests/_eig_ref.py (no GPU).

The default arithmetic of the kernels is bit-identical to the oracle (test_gpu_qr.py, test_gpu_qr_large_orders.py,
test_gpu_eig_sym_accuracy.py), so what the oracle gets wrong the kernels get wrong with it and no parity test
notices.  Here the oracle itself is scored, record by record against that record's own 2-norm, on hard spectra,
across the whole exponent range of the dtype and on subnormal input: within C everywhere except in the cells of
REFERENCE_EXCEEDS (upstream's arithmetic on repeated / clustered / rank-one spectra in float32), and really
above C in those, so that the list cannot rot or grow silently."""
import numpy as np
import pytest
import _eig_ref as E


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', E.ORDERS)
def test_oracle_per_record(oracle, dn, n):
    a, cells = E.batch(dn, n)
    assert len(a) % 64 != 0 and np.isfinite(a).all()
    vals, vals_u, vecs = E.oracle_results(oracle, dn, n)
    worst = E.per_cell(dn, n, E.judge(dn, n, vals, vals_u, vecs))
    for (cell, metric), r in sorted(worst.items(), key=lambda kv: -kv[1])[:6]:
        print(f'eig_sym oracle | {dn} | {n} | {cell} | {metric} | {r:.3g}')
    over = E.exceeding(dn, n, worst)
    assert over == E.listed(dn, n), (sorted(over - E.listed(dn, n)), sorted(E.listed(dn, n) - over))


def test_exclusions_are_few_and_never_a_scale():
    """no scale-sweep, subnormal or exact-zero cell may be excused, no float64 cell is, and every entry names a
    cell that exists"""
    assert len(E.REFERENCE_EXCEEDS) <= 24
    for dn, n, cell, metric in E.REFERENCE_EXCEEDS:
        assert dn == 'f32' and n in E.ORDERS and metric in E.METRICS
        assert cell in ('repeated', 'cluster', 'rank1', 'wilk'), cell
        assert not E.is_sweep(cell)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_shuffled_copy_is_the_same_records(oracle, dn):
    """the oracle works record by record: both copies of a cell hold the same records and get the same bits"""
    n = 5
    a, cells = E.batch(dn, n)
    vals = E.oracle_results(oracle, dn, n)[0]
    for idx in cells.values():
        h = len(idx) // 2
        assert np.array_equal(a[idx[:h]], a[idx[h:]]) and np.array_equal(vals[idx[:h]], vals[idx[h:]], equal_nan=True)
    # wavefronts of the shuffled copy mix the cells
    nb = len(a) // 2
    owner = np.empty(len(a), np.int64)
    for k, idx in enumerate(cells.values()):
        owner[idx] = k
    assert all(len(set(owner[s:s + 64])) > 8 for s in range(nb, len(a) - 64, 64))


def test_judges_notice_a_small_wrong_record():
    """a record 2^-60 of its neighbours' size that is entirely wrong: invisible to a batch-wide relative error,
    inf / large here; and the judges pass the float64 eigendecomposition rounded to the dtype"""
    dn, n = 'f32', 4
    a = E.batch(dn, n)[0]
    tr = E.truth(dn, n)
    lam, u = np.linalg.eigh(tr[1])
    vals = np.ldexp(lam, tr[0][:, None]).astype(np.float32)
    vecs = u.astype(np.float32)
    good = E.judge(dn, n, vals, vals, vecs)
    assert all(r.max() <= 2 for r in good.values()), {m: r.max() for m, r in good.items()}
    i = int(E.batch(dn, n)[1]['normal*2^-60'][0])
    bad = vals.copy()
    bad[i] = np.diagonal(a[i])                    # "deflated at once": the diagonal instead of the eigenvalues
    batch_wide = np.abs(bad.astype(np.float64) - vals).max() / np.abs(vals[np.isfinite(vals)]).max()
    assert batch_wide < 1e-30
    assert E.judge_values(dn, n, bad)[i] > 1e4
    bad[i] = np.nan
    assert E.judge_values(dn, n, bad)[i] == np.inf


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', [2, 3, 4, 5, 8, 9, 10, 11, 13, 15, 16])
def test_oracle_on_the_range_batches(oracle, dn, n):
    """the batch of test_gpu_qr.py::test_eig_sym_default_bits_across_ranges and of
    test_gpu_qr_large_orders.py::test_range_votes (1e-30 ... 1e18 / 1e-250 ... 1e140, zeros, denormal entries): those
    tests assert kernel == oracle bit for bit; this one that the oracle is RIGHT there, record by record"""
    import _qr_large_ref as R
    a = R.vote_batch(dn, n)[0]
    vals_u, vecs = oracle.eig_sym(a, True)
    E.assert_records_within(dn, n, a, oracle.eig_sym(a), vals_u, vecs)
