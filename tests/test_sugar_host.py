"""CPU-side checks of `sugar` (lmdiv / rmdiv / inv / solvevec and the torch compositions): the public surface is the
reference's, `compat` resolves its import paths, CPU tensors are refused, `nfm_sugar_solve` answers the bad calls
with the documented codes in the documented precedence, the code objects hold exactly the kernels the dispatch
reaches (none with a private segment), and the golden fixture agrees with numpy's float64 solves."""
import inspect
import os
import re
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT, GOLDEN, TOL, relerr

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
F32, F64, LU, CHOL = 0, 1, 0, 1
ORDERS = tuple(range(1, 9)) + (12,)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ public surface
# sugar.py of the reference: __all__ in its order, every function's parameters and defaults
SURFACE = {
    'kron2': [('a',), ('b',)],
    'lmdiv': [('a',), ('b',), ('method', 'lu'), ('rcond', 1e-15), ('out', None)],
    'rmdiv': [('a',), ('b',), ('method', 'lu'), ('rcond', 1e-15), ('out', None)],
    'inv': [('a',), ('method', 'lu'), ('rcond', 1e-15), ('out', None)],
    'matvec': [('mat',), ('vec',), ('out', None)],
    'solvevec': [('mat',), ('vec',), ('method', 'lu'), ('rcond', 1e-15), ('out', None)],
    'outer': [('a',), ('b',), ('out', None)],
    'trace': [('a',), ('keepdim', False)],
    'dot': [('a',), ('b',), ('keepdim', False), ('out', None)],
    'mdot': [('a',), ('b',), ('keepdim', False), ('out', None)],
    'is_orthonormal': [('basis',), ('return_matrix', False)],
    'round': [('t',), ('decimals', 0)],
}


def test_public_surface_is_the_reference():
    from nitorch_fastmath_amd import sugar as S
    assert S.__all__ == list(SURFACE)
    for name, params in SURFACE.items():
        sig = inspect.signature(getattr(S, name)).parameters
        assert list(sig) == [p[0] for p in params], name
        for p in params:
            d = sig[p[0]].default
            assert (d is inspect.Parameter.empty) if len(p) == 1 else (d == p[1] and type(d) is type(p[1])), (name, p)


def test_compat_resolves_sugar():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        nf = importlib.import_module('nitorch_fastmath')
        from nitorch_fastmath.sugar import lmdiv, rmdiv, inv, solvevec
        import nitorch_fastmath.sugar as ns
        import nitorch_fastmath_amd as N
        assert ns is N.sugar and lmdiv is N.sugar.lmdiv and rmdiv is N.sugar.rmdiv
        assert inv is N.sugar.inv and solvevec is N.sugar.solvevec
        for name in SURFACE:                    # star-imported, as upstream's __init__ does
            assert getattr(nf, name) is getattr(N.sugar, name), name
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)


def test_cpu_tensors_are_refused():
    from nitorch_fastmath_amd import sugar as S
    a, b, v = torch.eye(3).expand(4, 3, 3), torch.ones(4, 3, 2), torch.ones(4, 3)
    calls = [lambda: S.lmdiv(a, b), lambda: S.lmdiv(a, b, 'chol'), lambda: S.lmdiv(a, b, 'svd'),
             lambda: S.rmdiv(b.transpose(-1, -2), a), lambda: S.inv(a), lambda: S.inv(a, 'chol'),
             lambda: S.solvevec(a, v), lambda: S.matvec(a, v), lambda: S.kron2(a, b), lambda: S.outer(v, v),
             lambda: S.trace(a), lambda: S.dot(v, v), lambda: S.mdot(a, a), lambda: S.is_orthonormal(a[0]),
             lambda: S.round(a), lambda: S.lmdiv(torch.eye(12)[None], torch.ones(1, 12, 2))]
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(ValueError, match='Unknown inversion method'):
        S._method('qr', a)
    assert S._method('LU_anything', a) == 'lu' and S._method('Cholesky', a) == 'chol'
    assert S._method('lu', b) == 'pinv'                     # non-square: always the pseudo-inverse


def test_column_blocks_of_the_shared_solve_path(L, monkeypatch):
    """the split of k columns at `cap` per launch; with the launch helper counted (nothing runs: CPU tensors never
    reach a kernel), a k that fits is one launch on a, b and out themselves, a wider one a launch per block on views"""
    from nitorch_fastmath_amd import sugar as S
    assert S._blocks(8, 8) == [(0, 8)] and S._blocks(8, 6) == [(0, 6), (6, 8)] and S._blocks(1, 4) == [(0, 1)]
    assert S._blocks(11, 8) == [(0, 8), (8, 11)] and S._blocks(12, 4) == [(0, 4), (4, 8), (8, 12)]
    seen = []
    monkeypatch.setattr(S, '_launch', lambda family, dev, dtype, scalars, a, b, out: seen.append((scalars, a, b, out)))
    a, a12 = torch.zeros(5, 8, 8, dtype=torch.float64), torch.zeros(5, 12, 8, dtype=torch.float64)
    for family, sys_, flag, cap in ((S._SQUARE, a, LU, S.max_cols(a.dtype, 8)), (S._SVD, a, 1, S.svd_max_cols(a.dtype, 8, 8)),
                                    (S._LSTSQ, a12, None, S.lstsq_max_cols(a.dtype, 8))):
        m = sys_.shape[-2]
        head = (lambda k: {S._SQUARE: (8, k, flag), S._SVD: (8, 8, k, flag, 0.5), S._LSTSQ: (12, 8, k, 0.5)}[family])
        b, out = torch.zeros(5, m, cap, dtype=a.dtype), torch.zeros(5, 8, cap, dtype=a.dtype)
        del seen[:]
        assert S._kernel_solve(family, sys_, b, out, flag, 0.5) is out and len(seen) == 1
        assert seen[0][0] == head(cap) and seen[0][1] is sys_ and seen[0][2] is b and seen[0][3] is out
        b, out = torch.zeros(5, m, cap + 2, dtype=a.dtype), torch.zeros(5, 8, cap + 2, dtype=a.dtype)
        del seen[:]
        S._kernel_solve(family, sys_, b, out, flag, 0.5)
        assert [(sc, tuple(x.shape), x.data_ptr() - out.data_ptr()) for sc, _, _, x in seen] == \
            [(head(cap), (5, 8, cap), 0), (head(2), (5, 8, 2), cap * 8)]
        assert [tuple(x.shape) for _, _, x, _ in seen] == [(5, m, cap), (5, m, 2)]
    del seen[:]                                           # the identity: one launch, k = n (lu, chol) or m (svd)
    assert S._kernel_solve(S._SQUARE, a, None, None, CHOL).shape == (5, 8, 8) and seen[0][0] == (8, 8, CHOL)
    assert S._kernel_solve(S._SVD, a12[:, :8, :3], None, None, 0, 0.5).shape == (5, 3, 8) and seen[1][0] == (8, 3, 8, 0, 0.5)
    assert len(seen) == 2 and seen[0][2] is None and seen[1][2] is None


# ------------------------------------------------------------------------------------------------ the C ABI
def solve(L, dtype=F32, N=3, K=3, flags=LU, no=1, ni=1, a=4096, b=4096, out=4096):
    st = (0, 1, 1, 1)
    return L.nfm_sugar_solve(dtype, N, K, flags, no, ni, a, *st, b, *st, out, *st, None)


def test_abi_sweep_of_nfm_sugar_solve(L):
    """every call here is refused (or is an empty batch) before any launch: the addresses are never read"""
    assert solve(L, dtype=7) == EDTYPE
    assert solve(L, ni=-1) == EINVAL and solve(L, no=-1) == EINVAL
    assert solve(L, no=65536) == ESIZE
    for bad in (0, 9):
        assert solve(L, N=bad) == ESIZE and solve(L, K=bad) == ESIZE
    assert solve(L, N=-1) == ESIZE and solve(L, K=17) == ESIZE
    assert solve(L, flags=2) == EINVAL and solve(L, flags=-1) == EINVAL
    assert solve(L, N=3, K=2, b=None) == EINVAL                      # identity right-hand side needs K == N
    assert solve(L, N=2, K=3, b=None, flags=CHOL) == EINVAL
    assert solve(L, a=None) == EINVAL and solve(L, out=None) == EINVAL
    assert solve(L, a=6) == EALIGN and solve(L, b=6) == EALIGN and solve(L, out=6) == EALIGN
    assert solve(L, dtype=F64, a=4100) == EALIGN and solve(L, dtype=F64, out=4100) == EALIGN
    assert solve(L, N=3, K=3, b=None, a=None) == EINVAL and solve(L, N=3, K=3, b=None, out=6, flags=CHOL) == EALIGN
    # two errors at once: the precedence of the header
    assert solve(L, dtype=7, N=9) == EDTYPE and solve(L, dtype=7, ni=-1) == EDTYPE
    assert solve(L, ni=-1, no=65536) == EINVAL and solve(L, ni=-1, N=9) == EINVAL
    assert solve(L, no=65536, flags=2) == ESIZE and solve(L, N=9, flags=2) == ESIZE and solve(L, K=0, a=None) == ESIZE
    assert solve(L, flags=2, a=6) == EINVAL and solve(L, N=3, K=2, b=None, a=6) == EINVAL
    assert solve(L, a=None, out=6) == EINVAL and solve(L, a=6, out=None) == EALIGN
    assert solve(L, a=6, b=None, K=3) == EALIGN and solve(L, b=6, out=None) == EALIGN
    # the empty batch: null pointers, no launch
    for flags in (LU, CHOL):
        assert solve(L, ni=0, a=None, b=None, out=None, flags=flags) == OK
        assert solve(L, no=0, a=None, b=None, out=None, flags=flags, dtype=F64, N=8, K=1) == OK
    assert solve(L, ni=0, N=9, a=None, b=None, out=None) == ESIZE
    # more columns than one launch takes at this order: the caller solves in blocks
    from nitorch_fastmath_amd import sugar as S
    for dt, code in ((torch.float32, F32), (torch.float64, F64)):
        for N in range(1, 9):
            cap = L.nfm_sugar_max_cols(code, N)
            assert 1 <= cap <= 8 and S.max_cols(dt, N) == cap
            assert solve(L, dtype=code, N=N, K=cap, ni=0, a=None, b=None, out=None) == OK
            if cap < 8:
                assert solve(L, dtype=code, N=N, K=cap + 1) == ESIZE
    assert L.nfm_sugar_max_cols(7, 3) == EDTYPE and L.nfm_sugar_max_cols(F32, 0) == ESIZE
    assert L.nfm_sugar_max_cols(F64, 9) == ESIZE
    assert L.nfm_version() == 5


# ------------------------------------------------------------------------------------------------ code objects
def _census():
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_sugar*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    return KR.collect(objs)


def test_sugar_kernels_in_the_census(L):
    """every (dtype, method, N, K) up to the column cap has its kernels -- the run-time-mode, contiguous and
    channel-first kinds --, none has scratch, and nothing beyond the caps is compiled"""
    rows = _census()
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    assert max(k['vgpr'] for k in rows) <= 512
    seen = {}
    for k in rows:
        m = re.match(r'rec_kernel<(float|double), (SolveLuOp|SolveCholOp|CholInvOp)<(?:float|double), (\d+)(?:, (\d+))?>, (\d)>$',
                     k['kernel'])
        assert m, k['kernel']                       # no other kernel lives in these objects
        t, op, N, K, kind = m.groups()
        seen.setdefault((t, op, int(N), int(K) if K else None), set()).add(int(kind))
    want = set()
    for t, code in (('float', F32), ('double', F64)):
        for N in range(1, 9):
            want.add((t, 'CholInvOp', N, None))
            for K in range(1, L.nfm_sugar_max_cols(code, N) + 1):
                want |= {(t, 'SolveLuOp', N, K), (t, 'SolveCholOp', N, K)}
    assert set(seen) == want, sorted(set(seen) ^ want)[:8]
    assert all(kinds >= {0, 1, 2} for kinds in seen.values())


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_golden_agrees_with_numpy_float64(dn):
    g = np.load(os.path.join(GOLDEN, 'sugar.npz'))
    assert os.path.getsize(os.path.join(GOLDEN, 'sugar.npz')) < 1 << 20
    for N in ORDERS:
        def G(k):
            return g[f'{dn}_{N}_{k}']
        a, spd, b, v, ar = (G(k).astype(np.float64) for k in ('a', 'spd', 'b', 'v', 'ar'))
        assert G('a').dtype == (np.float32 if dn == 'f32' else np.float64) and a.shape == (16, N, N) and b.shape == (16, N, 3)
        x = np.linalg.solve(a, b)
        for m in ('lu', 'svd', 'pinv'):
            assert relerr(G('lmdiv_' + m), x) <= TOL[dn], (N, m)
            assert relerr(G('inv_' + m), np.linalg.inv(a)) <= TOL[dn], (N, m)
        assert relerr(G('lmdiv_chol'), np.linalg.solve(spd, b)) <= TOL[dn], N
        assert relerr(G('inv_chol'), np.linalg.inv(spd)) <= TOL[dn], N
        assert relerr(G('solvevec'), np.linalg.solve(a, v[..., None])[..., 0]) <= TOL[dn], N
        # the two expectations that are numpy's own: X a = ar, and the inverse of one SPD matrix
        assert G('rmdiv').dtype == np.float64 and relerr(G('rmdiv') @ a, ar) <= 1e-13
        assert relerr(G('inv_chol_2d') @ spd[0], np.eye(N)) <= 1e-13
        assert relerr(G('trace'), np.trace(a, axis1=1, axis2=2)) <= TOL[dn]
        assert relerr(G('dot'), (v * b[..., 0]).sum(-1)) <= TOL[dn] and relerr(G('mdot'), (a * spd).sum((-1, -2))) <= TOL[dn]
        assert relerr(G('outer'), v[:, :, None] * G('w').astype(np.float64)[:, None, :]) <= TOL[dn]
        kr = G('kron2')
        assert kr.shape == (N * N, 3 * N)
        # the reference's layout: [p, m, q, n] = a[m, n] b[p, q]
        assert relerr(kr.reshape(N, N, 3, N), np.einsum('mn,pq->pmqn', a[0], b[0])) <= TOL[dn]
        assert relerr(G('round'), np.round(a * 100) / 100) <= TOL[dn]
