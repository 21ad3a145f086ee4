"""CPU-side checks of `batched.batchsvdvals`, `batchsvd`, `batchpolar`: the record routine of the kernels through
`nfm_polar_host` (the same source, compiled for the host) against the bounds of tests/_polar_ref.py on every family,
the compiled caps and the code-object census, the C ABI's answers without a GPU, the facade on CPU tensors (the torch
compositions of `_polar.py`), and the fixture against mpmath."""
import ctypes
import glob
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _polar_ref as R

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
OPS = {R.VALS: 'SvdValsOp', R.FULL: 'SvdFullOp', R.POLAR: 'PolarOp', R.BWD: 'PolarBwdOp'}
ENTRIES = ('nfm_batch_svdvals', 'nfm_batch_svd', 'nfm_batch_polar', 'nfm_batch_polar_backward')
CASES = [(dn, n) for dn in ('f32', 'f64') for n in R.ORDERS]


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_bound(L):
    from nitorch_fastmath_amd import _lib, batched
    for name in ENTRIES + ('nfm_polar_max_order', 'nfm_polar_host'):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name]
        assert ctypes.POINTER(_lib.Operand) not in _lib.SIGNATURES[name]
    hdr = open(os.path.join(ROOT, 'include', 'nfm_hip.h')).read()
    for k, v in (('SVDVALS', 0), ('SVD', 1), ('POLAR', 2), ('POLAR_BACKWARD', 3)):
        assert f'#define NFM_POLAR_OP_{k} {v}\n' in hdr
    for name in ('batchsvdvals', 'batchsvd', 'batchpolar'):
        assert name in batched.__all__


def test_caps(L):
    from nitorch_fastmath_amd import batched
    for dn in ('f32', 'f64'):
        for op, name in ((R.VALS, 'svdvals'), (R.FULL, 'svd'), (R.POLAR, 'polar'), (R.BWD, 'polar_backward')):
            cap = L.nfm_polar_max_order(R.CODE[dn], op)
            assert 4 <= cap <= 8, (dn, op, cap)
            assert batched.polar_max_order(R.TT[dn], name) == cap
    assert L.nfm_polar_max_order(7, 0) == 0 and L.nfm_polar_max_order(0, 4) == 0 and L.nfm_polar_max_order(1, -1) == 0


def _call(L, entry, dtype=0, N=3, no=1, ni=1, ops=None, ptr=4096):
    from nitorch_fastmath_amd import _lib
    n_op = 4 if entry == 3 else 2
    ops = [_lib.Operand(ptr, 0, 1, 0, 1) for _ in range(n_op)] if ops is None else ops
    refs = [None if o is None else ctypes.byref(o) for o in ops]
    return getattr(L, ENTRIES[entry])(dtype, N, no, ni, *refs, None)


@pytest.mark.parametrize('entry', [0, 1, 2, 3])
def test_argument_errors_without_a_gpu(L, entry):
    """the canonical bad calls of tests/test_abi_sweep_host.py with the codes and the precedence of nfm_batch_det, then
    the entry's own checks; every call is refused (or is an empty batch) before any launch"""
    from nitorch_fastmath_amd import _lib
    n_op = 4 if entry == 3 else 2
    good = lambda: _lib.Operand(4096, 0, 1, 0, 1)                      # noqa: E731
    assert _call(L, entry, dtype=7) == EDTYPE
    assert _call(L, entry, ni=-1) == EINVAL
    assert _call(L, entry, no=65536) == ESIZE
    assert _call(L, entry, N=0) == ESIZE and _call(L, entry, N=17) == ESIZE
    required = (0, 3) if entry == 3 else (0, 1)          # the cotangents of the backward entry are optional
    for k in required:
        with_k = lambda o: [o if i == k else good() for i in range(n_op)]          # noqa: E731
        assert _call(L, entry, ops=with_k(None)) == EINVAL
        assert _call(L, entry, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
        assert _call(L, entry, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    if entry == 3:
        assert _call(L, entry, ops=[good(), None, None, good()]) == EINVAL          # no cotangent at all
        for k in (1, 2):          # a cotangent that is given is checked like every operand
            with_k = lambda o: [o if i == k else good() for i in range(n_op)]          # noqa: E731
            assert _call(L, entry, ops=with_k(_lib.Operand(None, 0, 1, 0, 1))) == EINVAL
            assert _call(L, entry, ops=with_k(_lib.Operand(6, 0, 1, 0, 1))) == EALIGN
    assert _call(L, entry, dtype=7, N=17) == EDTYPE
    assert _call(L, entry, N=17, ops=[None] + [good() for _ in range(n_op - 1)]) == ESIZE
    assert _call(L, entry, dtype=7, ops=[None] + [good() for _ in range(n_op - 1)]) == EDTYPE
    assert _call(L, entry, ni=0, ptr=None) == OK
    for dn in ('f32', 'f64'):
        cap = L.nfm_polar_max_order(R.CODE[dn], entry)
        assert _call(L, entry, dtype=R.CODE[dn], N=cap, ni=0) == OK
        assert _call(L, entry, dtype=R.CODE[dn], N=cap + 1, ni=0) == ESIZE


def test_host_entry_argument_errors(L):
    x = np.ones(64)
    p = x.ctypes.data
    assert L.nfm_polar_host(7, 0, 2, 1, p, None, None, p) == EDTYPE
    assert L.nfm_polar_host(1, 4, 2, 1, p, None, None, p) == EINVAL
    assert L.nfm_polar_host(1, 0, 2, -1, p, None, None, p) == EINVAL
    assert L.nfm_polar_host(1, 0, 0, 1, p, None, None, p) == ESIZE and L.nfm_polar_host(1, 0, 9, 1, p, None, None, p) == ESIZE
    assert L.nfm_polar_host(1, 0, 2, 1, None, None, None, p) == EINVAL
    assert L.nfm_polar_host(1, 3, 2, 1, p, None, None, p) == EINVAL
    assert L.nfm_polar_host(1, 0, 2, 0, None, None, None, None) == OK


# ------------------------------------------------------------------------------------------------ the census
def test_polar_kernels_in_the_census(L):
    """every (dtype, op, N <= cap) is compiled, none beyond the cap, none with a private segment"""
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_polar_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    rows = KR.collect(objs)
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    names = [k['kernel'] for k in rows]
    for dn, t in (('f32', 'float'), ('f64', 'double')):
        for code, op in OPS.items():
            cap = L.nfm_polar_max_order(R.CODE[dn], code)
            for N in range(1, 10):
                have = any(f'{op}<{t}, {N}>' in n for n in names)
                assert have == (N <= cap), (dn, op, N, cap)


# ------------------------------------------------------------------------------------------------ the record routine
@pytest.mark.parametrize('dn,n', CASES)
def test_forward_bounds_through_the_host_entry(L, dn, n):
    """every family; float32 against numpy's float64 SVD on the whole batch, float64 against the mpmath fixture on its
    records and by the truth-free bounds everywhere.  The largest sweep count is printed."""
    a, _ = R.batch(dn, n)
    S, sw0 = R.host(L, R.VALS, a)
    full, sw1 = R.host(L, R.FULL, a)
    pol, sw2 = R.host(L, R.POLAR, a)
    print(f'{dn} {n}x{n}: largest sweep count {max(sw0, sw1, sw2)}')
    assert max(sw0, sw1, sw2) < 16
    U, S2, Vh = R.split_full(full, n)
    assert np.array_equal(S, S2), 'the values kernel and the full kernel run the same sweeps'
    worst = R.report(f'host {dn} {n}x{n}', R.forward_ratios(dn, n, S, (U, S2, Vh), R.split_polar(pol, n)))
    assert worst <= 1.0


@pytest.mark.parametrize('dn,n', CASES)
def test_gradient_bounds_through_the_host_entry(L, dn, n):
    a, _, gr, gp, gs, _, _, _ = R.grad_cases(dn, n)
    sh = lambda x: x[0].reshape(-1, n, n)          # noqa: E731
    U, _, Vh = R.split_full(R.host(L, R.FULL, a)[0], n)
    ratios = R.grad_ratios(dn, n, sh(R.host(L, R.BWD, a, gr, None)), sh(R.host(L, R.BWD, a, None, gp)),
                           sh(R.host(L, R.BWD, a, gr, gp)), (U * gs[:, None, :]) @ Vh)
    assert R.report(f'host gradient {dn} {n}x{n}', ratios) <= 1.0


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_bad_records_stay_alone(L, dn):
    a = np.array(R.batch(dn, 3)[0][:8])
    a[2, 1, 1], a[5, 0, 2] = np.nan, np.inf
    clean = np.array(R.batch(dn, 3)[0][:8])
    for op in (R.VALS, R.FULL, R.POLAR):
        got, ref = R.host(L, op, a)[0], R.host(L, op, clean)[0]
        assert np.isnan(got[[2, 5]]).all()
        keep = [0, 1, 3, 4, 6, 7]
        assert np.array_equal(got[keep], ref[keep])
    g = np.ones_like(a)
    got = R.host(L, R.BWD, a, g, g)[0]
    assert np.isnan(got[[2, 5]]).all() and np.isfinite(got[[0, 1, 3, 4, 6, 7]]).all()


# ------------------------------------------------------------------------------------------------ the facade on the CPU
@pytest.mark.parametrize('dn,n', [(dn, n) for dn in ('f32', 'f64') for n in (1, 3, 8, 9)])
def test_facade_on_cpu_tensors(L, dn, n):
    """CPU tensors take the torch compositions; they meet the bounds the host entry is held to (n = 9: above every
    cap, by the truth-free bounds)"""
    from nitorch_fastmath_amd import batched as B
    if n in R.ORDERS:
        a = torch.from_numpy(np.array(R.batch(dn, n)[0]))
        S = B.batchsvdvals(a).numpy()
        svd = tuple(x.numpy() for x in B.batchsvd(a))
        pol = tuple(x.numpy() for x in B.batchpolar(a))
        assert R.report(f'cpu facade {dn} {n}x{n}', R.forward_ratios(dn, n, S, svd, pol)) <= 1.0
        left = B.batchpolar(a, side='left')
        tr = B.batchpolar(a.transpose(-1, -2))
        assert torch.equal(left[0], tr[0].transpose(-1, -2)) and torch.equal(left[1], tr[1])
        # autograd on the CPU route against the fixture
        af, _, gr, gp, gs, _, _, _ = R.grad_cases(dn, n)
        t = lambda x: torch.from_numpy(np.array(x))          # noqa: E731
        x = t(af).requires_grad_()
        Rr, P = B.batchpolar(x)
        (g3,) = torch.autograd.grad([Rr, P], x, [t(gr), t(gp)])
        x = t(af).requires_grad_()
        (g1,) = torch.autograd.grad(B.batchpolar(x)[0], x, t(gr))
        x = t(af).requires_grad_()
        (g2,) = torch.autograd.grad(B.batchpolar(x)[1], x, t(gp))
        x = t(af).requires_grad_()
        (g4,) = torch.autograd.grad(B.batchsvdvals(x), x, t(gs))
        ratios = R.grad_ratios(dn, n, g1.numpy(), g2.numpy(), g3.numpy(), g4.numpy())
        assert R.report(f'cpu facade gradient {dn} {n}x{n}', ratios) <= 1.0
    else:
        a = np.random.default_rng(9).standard_normal((50, n, n)).astype(R.NP[dn])
        U, S, Vh = (x.numpy() for x in B.batchsvd(torch.from_numpy(a)))
        Rr, P = (x.numpy() for x in B.batchpolar(torch.from_numpy(a)))
        ratios = R.svd_ratios(dn, a, U, S, Vh)
        pr, sym = R.polar_self_ratios(dn, a, Rr, P, S[:, 0])
        ratios.update(pr)
        assert sym and R.ordered(S) and R.report(f'cpu facade {dn} {n}x{n}', ratios) <= 1.0


def test_facade_argument_errors():
    from nitorch_fastmath_amd import batched as B
    with pytest.raises(ValueError):
        B.batchpolar(torch.zeros(3, 2, 3))
    with pytest.raises(ValueError):
        B.batchpolar(torch.zeros(3, 2, 2), side='up')
    with pytest.raises(TypeError):
        B.batchsvdvals(torch.zeros(3, 2, 2, dtype=torch.float16))
    # batchsvd with a gradient is torch.linalg.svd, forward and backward
    x = torch.eye(2, dtype=torch.float64).mul(2.0).add(torch.tensor([[0.0, 0.1], [0.0, 0.0]])).requires_grad_()
    U, S, Vh = B.batchsvd(x)
    assert S.grad_fn is not None and 'Svd' in type(S.grad_fn).__name__


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_present_and_matches_mpmath():
    assert os.path.getsize(R.FIXTURE) < 400 * 1024
    fx = R.fixture()
    for dn in ('f32', 'f64'):
        for n in R.ORDERS:
            for fam in R.FAMILIES:
                assert np.array_equal(fx[f'{dn}_{n}_{fam}_a'], R.family(fam, n, R.NFIX, dn)), (dn, n, fam)
                for k in ('S', 'R', 'P', 'gaR', 'gaP', 'gaS'):
                    assert fx[f'{dn}_{n}_{fam}_{k}'].dtype == np.float64
    mp = pytest.importorskip('mpmath')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    try:
        import make_golden_polar as G
    finally:
        sys.path.pop(0)
    for dn, n, fam, k in (('f64', 3, 'cluster', 1), ('f32', 4, 'repeated', 0), ('f64', 2, 'negdet', 2)):
        a = R.family(fam, n, R.NFIX, dn)[k]
        gr, gp, _ = R.cotangents(n, R.NFIX, dn, fam)
        A = G.to_mp(a)
        U, S, Vh = G.decompose(A)
        assert np.array_equal(np.array([float(s) for s in S]), R.fix(dn, n, fam, 'S')[k])
        assert np.allclose(G.to_np(Vh.T * mp.diag(S) * Vh), R.fix(dn, n, fam, 'P')[k], rtol=0, atol=1e-15 * float(S[0]))
        assert np.allclose(G.to_np(G.polar_grad(A, G.to_mp(gr[k]), None)), R.fix(dn, n, fam, 'gaR')[k], rtol=1e-13)
        if n <= 3:
            assert G.check_form(A, G.to_mp(gr[k]), G.to_mp(gp[k])) < mp.mpf(10) ** -15
