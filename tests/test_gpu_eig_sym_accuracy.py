"""eig_sym on the GPU held to the per-record bars of tests/_eig_ref.py: hard spectra (repeated, clustered,
rank-one, graded, Wilkinson), the whole exponent range of the dtype, subnormal input and the exact-zero
structures, 64 records per cell, once cell by cell and once shuffled record by record so that every wavefront
mixes scales and families (every range decision of nfm_qr_core.hpp is a wavefront vote).

Per (dtype, order, storage form): the values-only kernel and the kernel with vectors (different kernels: the
"stuck" exit exists only in the first), contiguous records and a matrix-first view (orders 9..16: the register
form and the LDS-resident form).
  arithmetic='reference'  bit-identical to the oracle on the whole batch, hence within C exactly where the oracle
                          is (test_eig_sym_accuracy_host.py): everywhere but REFERENCE_EXCEEDS;
  arithmetic='fast'       within C in EVERY cell, no exclusions, and the two kernels return the same set of
                          eigenvalues within 2 C n eps |A|_2.
Each test prints its worst cells; profiles/eig_sym_accuracy.md has every cell
(scripts/eig_sym_accuracy_scan.py)."""
import pytest
from test_gpu_qr_large_orders import Form
import _qr_large_ref as R
import _eig_ref as E

pytestmark = pytest.mark.gpu


def run(dev, form, mode, a):
    F = Form(dev, form, mode)
    vals = F.eig_sym(a)
    vals_u, vecs = F.eig_sym(a, True)
    assert F.unchanged()
    return vals, vals_u, vecs


def report(dn, n, form, mode, worst):
    for (cell, metric), r in sorted(worst.items(), key=lambda kv: -kv[1])[:5]:
        print(f'eig_sym accuracy | {dn} | {n} | {form} | {mode} | {cell} | {metric} | {r:.3g}')


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', E.ORDERS)
@pytest.mark.parametrize('form', ['contiguous', 'matrix-first'])
def test_reference_arithmetic(dev, oracle, dn, n, form):
    a = E.batch(dn, n)[0]
    ref = E.oracle_results(oracle, dn, n)
    got = run(dev, form, 'reference', a)
    worst = E.per_cell(dn, n, E.judge(dn, n, *got))
    report(dn, n, form, 'reference', worst)
    for name, x, y in zip(('values', 'values (vectors call)', 'vectors'), got, ref):
        assert R.same_bits(x, y), (name, R.worst_record(x, y))
    over = E.exceeding(dn, n, worst)
    assert over == E.listed(dn, n), (sorted(over - E.listed(dn, n)), sorted(E.listed(dn, n) - over))


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', E.ORDERS)
@pytest.mark.parametrize('form', ['contiguous', 'matrix-first'])
def test_fast_arithmetic(dev, dn, n, form):
    a, cells = E.batch(dn, n)
    vals, vals_u, vecs = run(dev, form, 'fast', a)
    worst = E.per_cell(dn, n, E.judge(dn, n, vals, vals_u, vecs))
    report(dn, n, form, 'fast', worst)
    same = E.same_value_set(dn, n, vals, vals_u)
    sets = {c: float(same[idx].max()) for c, idx in cells.items()}
    c = max(sets, key=sets.get)
    print(f'eig_sym accuracy | {dn} | {n} | {form} | fast | {c} | value sets | {sets[c]:.3g}')
    over = E.exceeding(dn, n, worst)
    assert not over, sorted((x, worst[x[2:]]) for x in over)
    assert sets[c] <= 2 * E.C, (c, sets[c])
