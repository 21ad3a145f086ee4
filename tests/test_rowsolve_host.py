"""CPU-side checks of the square solves of orders 9..16 (`nfm_rowsolve`, the fourth kernel family of `sugar`):
the entry point answers the bad calls with the documented codes in the documented precedence before any launch,
`sugar` routes orders 9..16 with 'lu' / 'chol' to the family (and nothing else), and the code objects hold exactly
the kernels the dispatch reaches -- one form per (dtype, order), none with a private segment."""
import os
import re
import sys
import pytest
import torch
from conftest import ROOT

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
F32, F64, LU, CHOL = 0, 1, 0, 1
ORDERS = tuple(range(9, 17))
WIDTHS = (1, 2, 4, 8)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def solve(L, dtype=F32, N=12, K=3, flags=LU, no=1, ni=1, a=4096, b=4096, out=4096):
    st = (0, 1, 1, 1)
    return L.nfm_rowsolve(dtype, N, K, flags, no, ni, a, *st, b, *st, out, *st, None)


def test_abi_sweep_of_nfm_rowsolve(L):
    """every call here is refused (or is an empty batch) before any launch: the addresses are never read"""
    assert solve(L, dtype=7) == EDTYPE
    assert solve(L, ni=-1) == EINVAL and solve(L, no=-1) == EINVAL
    assert solve(L, no=65536) == ESIZE
    for bad in (-1, 0, 1, 8, 17):
        assert solve(L, N=bad) == ESIZE, bad
    for bad in (-1, 0, 17):
        assert solve(L, K=bad) == ESIZE, bad
    assert solve(L, flags=2) == EINVAL and solve(L, flags=-1) == EINVAL
    assert solve(L, N=12, K=8, b=None) == EINVAL                     # identity right-hand side needs K == N
    assert solve(L, N=9, K=12, b=None, flags=CHOL) == EINVAL
    assert solve(L, K=9) == ESIZE and solve(L, K=16, N=16) == ESIZE   # above the cap with a b
    assert solve(L, a=None) == EINVAL and solve(L, out=None) == EINVAL
    assert solve(L, a=6) == EALIGN and solve(L, b=6) == EALIGN and solve(L, out=6) == EALIGN
    assert solve(L, dtype=F64, a=4100) == EALIGN and solve(L, dtype=F64, out=4100) == EALIGN
    assert solve(L, N=12, K=12, b=None, a=None) == EINVAL
    assert solve(L, N=12, K=12, b=None, out=6, flags=CHOL) == EALIGN and solve(L, N=12, K=12, b=None, out=6) == EALIGN
    # two errors at once: the precedence of the header
    assert solve(L, dtype=7, N=8) == EDTYPE and solve(L, dtype=7, ni=-1) == EDTYPE
    assert solve(L, ni=-1, no=65536) == EINVAL and solve(L, ni=-1, N=8) == EINVAL
    assert solve(L, no=65536, flags=2) == ESIZE and solve(L, N=8, flags=2) == ESIZE and solve(L, K=0, a=None) == ESIZE
    assert solve(L, flags=2, a=6) == EINVAL and solve(L, flags=2, K=9) == EINVAL
    assert solve(L, N=12, K=9, b=None, a=6) == EINVAL and solve(L, K=9, a=6) == ESIZE
    assert solve(L, a=None, out=6) == EINVAL and solve(L, a=6, out=None) == EALIGN
    assert solve(L, a=6, b=None, K=12) == EALIGN and solve(L, b=6, out=None) == EALIGN
    # the empty batch: null pointers, no launch
    for flags in (LU, CHOL):
        assert solve(L, ni=0, a=None, b=None, out=None, flags=flags) == OK
        assert solve(L, no=0, a=None, b=None, out=None, flags=flags, dtype=F64, N=16, K=1) == OK
    assert solve(L, ni=0, N=8, a=None, b=None, out=None) == ESIZE and solve(L, ni=0, N=17, a=None, b=None, out=None) == ESIZE
    assert solve(L, ni=0, K=9, a=None, b=None, out=None) == ESIZE
    # the column cap, and the orders of the two square families do not overlap
    from nitorch_fastmath_amd import sugar as S
    for dt, code in ((torch.float32, F32), (torch.float64, F64)):
        for N in ORDERS:
            cap = L.nfm_rowsolve_max_cols(code, N)
            assert cap == max(WIDTHS) and S.rowsolve_max_cols(dt, N) == cap
            assert solve(L, dtype=code, N=N, K=cap, ni=0, a=None, b=None, out=None) == OK
            assert solve(L, dtype=code, N=N, K=cap + 1) == ESIZE
            assert L.nfm_sugar_max_cols(code, N) == ESIZE
        for N in (-1, 0, 1, 8, 17):
            assert L.nfm_rowsolve_max_cols(code, N) == ESIZE, N
    assert L.nfm_rowsolve_max_cols(7, 12) == EDTYPE and L.nfm_rowsolve_max_cols(7, 3) == EDTYPE
    st = (0, 1, 1, 1)
    assert L.nfm_sugar_solve(F32, 9, 3, LU, 1, 1, 4096, *st, 4096, *st, 4096, *st, None) == ESIZE
    assert L.nfm_version() == 5


# ------------------------------------------------------------------------------------------------ routing
@pytest.fixture
def launches(monkeypatch):
    """`sugar._launch` replaced by a recorder: nothing runs (CPU tensors never reach a kernel)"""
    from nitorch_fastmath_amd import sugar as S
    seen = []
    monkeypatch.setattr(S, '_launch', lambda family, dev, dtype, scalars, a, b, out: seen.append((family, scalars, a, b, out)))
    # the facade refuses CPU tensors before it routes: let them through to the recorder
    from nitorch_fastmath_amd import _dispatch
    monkeypatch.setattr(_dispatch, 'require_gpu', lambda *tensors: tensors[0].device)
    return seen


@pytest.mark.parametrize('N', [9, 12, 16])
def test_orders_9_to_16_reach_the_rowsolve_family(L, launches, N):
    from nitorch_fastmath_amd import sugar as S
    for dt in (torch.float32, torch.float64):
        a, b, v = torch.zeros(5, N, N, dtype=dt), torch.zeros(5, N, 3, dtype=dt), torch.zeros(5, N, dtype=dt)
        for method, flag in (('lu', LU), ('chol', CHOL)):
            del launches[:]
            x = S.lmdiv(a, b, method)
            assert x.shape == (5, N, 3) and len(launches) == 1
            fam, scalars, la, lb, lo = launches[0]
            assert fam is S._ROWSOLVE and scalars == (N, 3, flag) and la is a and lb is b and lo is x
            del launches[:]
            assert S.solvevec(a, v, method).shape == (5, N)
            assert [(f is S._ROWSOLVE, sc) for f, sc, *_ in launches] == [(True, (N, 1, flag))]
            del launches[:]
            r = S.rmdiv(torch.zeros(5, 2, N, dtype=dt), a, method)
            assert r.shape == (5, 2, N)
            (fam, scalars, la, lb, lo), = launches
            assert fam is S._ROWSOLVE and scalars == (N, 2, flag)
            assert la.stride()[-2:] == (1, N) and lb.shape == (5, N, 2) and lb.stride()[-2:] == (1, N)
        # k = cap + 3: one launch per block of columns, on views of b and of the result
        cap = S.rowsolve_max_cols(dt, N)
        bw = torch.zeros(5, N, cap + 3, dtype=dt)
        del launches[:]
        x = S.lmdiv(a, bw)
        assert [(f is S._ROWSOLVE, sc, tuple(lb.shape), tuple(lo.shape), lo.data_ptr() - x.data_ptr(), lb.data_ptr() - bw.data_ptr())
                for f, sc, _, lb, lo in launches] == \
            [(True, (N, cap, LU), (5, N, cap), (5, N, cap), 0, 0),
             (True, (N, 3, LU), (5, N, 3), (5, N, 3), cap * x.element_size(), cap * x.element_size())]
        # inv('chol'): the identity; inv('lu') stays with batchinv
        del launches[:]
        assert S.inv(a, 'chol').shape == (5, N, N)
        (fam, scalars, _, lb, _), = launches
        assert fam is S._ROWSOLVE and scalars == (N, N, CHOL) and lb is None


def test_what_does_not_reach_the_rowsolve_family(L, launches, monkeypatch):
    from nitorch_fastmath_amd import sugar as S
    torch_route = []
    monkeypatch.setattr(S, '_torch_lmdiv', lambda a, b, method, rcond, out: torch_route.append(method) or b.clone())
    a17, b17 = torch.zeros(5, 17, 17), torch.zeros(5, 17, 3)
    for method in ('lu', 'chol'):
        S.lmdiv(a17, b17, method)                                    # order 17: the torch composition
    a12, b12 = torch.zeros(5, 12, 12), torch.zeros(5, 12, 3)
    for method in ('svd', 'pinv'):
        S.lmdiv(a12, b12, method)                                    # 'svd' / 'pinv' at order 12: not this family
    S.lmdiv(torch.zeros(5, 0, 0), torch.zeros(5, 0, 3))              # order 0
    assert torch_route == ['lu', 'chol', 'svd', 'pinv', 'lu'] and not launches
    a8, b8 = torch.zeros(5, 8, 8), torch.zeros(5, 8, 3)
    for method, flag in (('lu', LU), ('chol', CHOL)):
        del launches[:]
        S.lmdiv(a8, b8, method)                                      # order 8: the lane-per-system kernels, as before
        assert [(f is S._SQUARE, sc) for f, sc, *_ in launches] == [(True, (8, 3, flag))]
    del launches[:]
    S.inv(a8, 'chol')
    assert [(f is S._SQUARE, sc) for f, sc, *_ in launches] == [(True, (8, 8, CHOL))]
    assert S._square_family(8) is S._SQUARE and S._square_family(9) is S._ROWSOLVE and S._square_family(16) is S._ROWSOLVE
    assert S._square_family(17) is None and S._square_family(0) is None


# ------------------------------------------------------------------------------------------------ code objects
def test_rowsolve_kernels_in_the_census(L):
    """every (dtype, method, N, width, layout kind) the entry point can launch has its kernel and nothing else is
    compiled; a (dtype, N) has one form (rows per lane, pivot row through LDS or not); no scratch"""
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_rowsolve_*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    rows = KR.collect(objs)
    assert len(objs) == 16
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    assert max(k['vgpr'] + (k['agpr'] or 0) for k in rows) <= 512
    assert max(k['lds_static'] for k in rows) <= 64 * 1024
    seen, forms = set(), {}
    for k in rows:
        m = re.match(r'rows::rowsolve_kernel<(float|double), (\d+), (\d+), (true|false), (\d), (true|false), (true|false)>$',
                     k['kernel'])
        assert m, k['kernel']                       # no other kernel lives in these objects
        t, N, KB, chol, R, lb, strided = m.groups()
        key = (t, 'chol' if chol == 'true' else 'lu', int(N), int(KB), 'strided' if strided == 'true' else 'contiguous')
        assert key not in seen, key
        seen.add(key)
        forms.setdefault((t, int(N)), set()).add((int(R), lb))
    want = {(t, method, N, KB, kind) for t in ('float', 'double') for method in ('lu', 'chol') for N in ORDERS
            for KB in WIDTHS for kind in ('contiguous', 'strided')}
    assert seen == want, sorted(seen ^ want)[:8]
    assert all(len(f) == 1 and next(iter(f))[0] in (1, 2, 4) for f in forms.values()), forms
