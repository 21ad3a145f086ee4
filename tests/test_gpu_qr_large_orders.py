"""The QR family (eig_sym, hessenberg, hessenberg_sym, qr_hessenberg, rq_hessenberg, householder and the two
apply operations) at EVERY order 9..16, both dtypes, on a thousand records, in both kernel forms of
nfm_qr.hip: the register form (`qr_large_*`, contiguous operands, where `qr_large_fits` allows) and the
LDS-resident form (`qr_lds_kernel`: every other order, and any operand that is not a one-level batch of
back-to-back records).  The rule of test_gpu_large_orders.py applies: these kernels live far beyond 256
registers per lane, where a toolchain slip shows up as wrong values in SOME lanes, so small batches are not
enough.

The bars are those of test_gpu_qr.py::test_vs_oracle (tests/_qr_large_ref.py); test_qr_large_orders_host.py
shows that the oracle alone meets them on the same inputs.  Between the two kernel forms the bar is bit
identity: both instantiate the same nfm_qr_core.hpp templates, the reference-order paths carry
`#pragma clang fp contract(off)` and the fast paths spell out their fmas.

Every test prints one `parity` line per (dtype, order, form, operation): the worst relerr against the oracle and
whether the result was bit-identical to the oracle / to the contiguous call; profiles/qr_large_orders_parity.md is
assembled from them."""
import numpy as np
import pytest
import torch
from conftest import relerr
from test_gpu_qr import GpuQ, Q, t, n_
import _qr_large_ref as R
import _eig_ref as E

pytestmark = pytest.mark.gpu
INT = {torch.float32: torch.int32, torch.float64: torch.int64}


class Form(GpuQ):
    """GpuQ whose operands reach the library in one storage form of _qr_large_ref.present, and which keeps a
    clone of every view it hands out: `unchanged()` compares them bit for bit after the calls"""

    def __init__(self, dev, form, arithmetic=None):
        super().__init__(dev, arithmetic)
        self.form, self.seen = form, []

    def t(self, x):
        view = R.present(t(x, self.dev), self.form)
        self.seen.append((view, view.clone()))
        return view

    def unchanged(self):
        ok = all(torch.equal(v.view(INT[v.dtype]), c.view(INT[c.dtype])) for v, c in self.seen)
        self.seen = []
        return ok


def emitter(dn, n, form):
    def emit(op, err, bits_oracle, bits_contiguous='self'):
        print(f'parity | {dn} | {n} | {op} | {form} | {err:.3g} | {bits_oracle} | {bits_contiguous}')
    return emit


def fast_lines(emit, fast, ref_eig, base=None):
    """the fast sweeps promise no order: their sorted values against the oracle's sorted values"""
    bits = R.family_bits(fast, base) if base is not None else {}
    for op, arrs in fast.items():
        ref = ref_eig[op][0]
        emit(op.replace('eig_sym', 'eig_sym fast'), relerr(np.sort(arrs[0], -1), np.sort(ref, -1)),
             R.same_bits(arrs[0], ref), bits.get(op, 'self'))


def all_bits(got, want):
    bits = R.family_bits(got, want)
    assert all(bits.values()), [op for op, b in bits.items() if not b]
    return bits


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.ORDERS)
def test_every_order_contiguous(dev, oracle, dn, n):
    """contiguous operands (the register form where it fits, the LDS form elsewhere), every operation twice -- a
    lane-dependent slip is rarely identical from run to run: TOL against the oracle position by position, default
    arithmetic = 'reference' bit for bit, eigenpairs and the error model in both arithmetic modes, Q R = H,
    P x = alpha e_b"""
    r, ax = R.records(dn, n), R.aux(oracle, dn, n)
    ref_eig, ref_rest = R.oracle_family(oracle, dn, n)
    emit = emitter(dn, n, 'contiguous')
    first = None
    for rep in range(2):
        G = GpuQ(dev)
        eig, rest = R.eig_family(G, r), R.rest_family(G, r, ax, n)
        R.check_tol({**eig, **rest}, {**ref_eig, **ref_rest}, dn, emit if rep == 0 else None)
        all_bits(R.eig_family(GpuQ(dev, 'reference'), r), eig)
        R.check_eig(eig, ref_eig, dn, n)
        R.check_relations(rest, ref_rest, dn, n)
        fast = R.eig_family(GpuQ(dev, 'fast'), r)
        R.check_eig(fast, ref_eig, dn, n, fast=True)
        if rep == 0:
            fast_lines(emit, fast, ref_eig)
            first = {**eig, **rest, **{'fast ' + k: v for k, v in fast.items()}}
        else:
            all_bits({**eig, **rest, **{'fast ' + k: v for k, v in fast.items()}}, first)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.ORDERS)
@pytest.mark.parametrize('form', R.FORMS)
def test_every_order_lds_form(dev, oracle, dn, n, form):
    """the same records as a matrix-first view ((n, n, nb) storage viewed as (nb, n, n); vectors (n, nb)) and as
    a two-level batch that does not collapse (torch.zeros(3, 340, n, n)[:, :337]: n_outer = 3, blockIdx.y, a
    ragged last tile in every slab): the register form answers NFM_EFALLBACK, the LDS-resident kernel runs.
    Bit-identical to the contiguous call for every operation and all three arithmetic settings, within the
    bars of test_every_order_contiguous against the oracle, and the input views unchanged."""
    r, ax, nb = R.records(dn, n), R.aux(oracle, dn, n), R.nb_of(n)
    ref_eig, ref_rest = (R.expected_of(x, form, nb) for x in R.oracle_family(oracle, dn, n))
    emit = emitter(dn, n, form)
    for mode in (None, 'reference', 'fast'):
        base = R.expected_of(R.eig_family(GpuQ(dev, mode), r), form, nb)
        F = Form(dev, form, mode)
        got = R.as_batch_first(R.eig_family(F, r), form)
        assert F.unchanged()
        bits = R.family_bits(got, base)
        if mode == 'fast':
            fast_lines(emit, got, ref_eig, base)
        elif mode is None:
            R.check_tol(got, ref_eig, dn, lambda op, e, b: emit(op, e, b, bits[op]))
        all_bits(got, base)
    base = R.expected_of(R.rest_family(GpuQ(dev), r, ax, n), form, nb)
    F = Form(dev, form)
    got = R.as_batch_first(R.rest_family(F, r, ax, n), form)
    assert F.unchanged()
    bits = R.family_bits(got, base)
    R.check_tol(got, ref_rest, dn, lambda op, e, b: emit(op, e, b, bits[op]))
    all_bits(got, base)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.ORDERS)
def test_rq_hessenberg_mixed_operands(dev, oracle, dn, n):
    """rq_hessenberg(h, u) with h contiguous and u matrix-first, and the converse: the second operand's strides.
    Bit-identical to the call on two contiguous operands."""
    r = R.records(dn, n)
    ref = R.oracle_family(oracle, dn, n)[1]['rq_hessenberg u']
    base = [n_(x) for x in Q().rq_hessenberg(t(r['hz'], dev), t(r['a'], dev))]
    for fh, fu in (('contiguous', 'matrix-first'), ('matrix-first', 'contiguous')):
        h, u = R.present(t(r['hz'], dev), fh), R.present(t(r['a'], dev), fu)
        h0, u0 = h.clone(), u.clone()
        got = [n_(x) for x in Q().rq_hessenberg(h, u)]
        assert torch.equal(h, h0) and torch.equal(u, u0)
        bits = all(R.same_bits(x, y) for x, y in zip(got, base))
        emitter(dn, n, f'h {fh}, u {fu}')('rq_hessenberg u', max(relerr(x, y) for x, y in zip(got, ref)),
                                         all(R.same_bits(x, y) for x, y in zip(got, ref)), bits)
        assert bits


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('n', R.VOTE_ORDERS)
@pytest.mark.parametrize('form', ['contiguous', 'matrix-first'])
def test_range_votes(dev, oracle, dn, n, form):
    """test_gpu_qr.py::test_eig_sym_default_bits_across_ranges at the register / LDS switch-over orders, through
    both forms: the default arithmetic takes the trimmed division / square-root sequences on a wavefront vote
    (nfm_qr_core.hpp, CrRange) and must give the oracle's bits whether a wavefront is in range, out of range or
    mixes both, on exact zeros, denormal entries and non-finite input.  arithmetic='fast' runs on the unit-scale
    wavefront and the exact-zero structures only: diagonal and zero records exact, the rest by eigenpairs and
    the error model."""
    a = R.vote_batch(dn, n)[0]
    ref, (rv, ru), ref_nf, ref_sub = R.vote_refs(oracle, dn, n)
    F = Form(dev, form)
    got = F.eig_sym(a)
    assert R.same_bits(got, ref), np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:8]
    gv, gu = F.eig_sym(a, True)
    assert R.same_bits(gv, rv) and R.same_bits(gu, ru)
    # right at every scale, record by record (tests/_eig_ref.py), not only equal to the oracle
    E.assert_records_within(dn, n, a, got, gv, gu)
    # non-finite input (check_finite=False): NaN where the oracle has NaN, everything else equal
    got = n_(Q().eig_sym(F.t(R.vote_nonfinite(a)), check_finite=False))
    assert np.array_equal(np.isnan(got), np.isnan(ref_nf))
    ok = ~np.isnan(ref_nf)
    assert np.array_equal(got[ok], ref_nf[ok])
    assert F.unchanged()
    F = Form(dev, form, 'fast')
    sub = R.vote_fast_subset(dn, n)[0]
    vals = F.eig_sym(sub)
    vals_u, vecs = F.eig_sym(sub, True)
    assert F.unchanged()
    R.check_fast_subset(vals, vals_u, vecs, ref_sub, dn, n)
