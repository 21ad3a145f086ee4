"""CPU-side checks of the Jacobi SVD solves (`nfm_svd_solve`, `nfm_svd_solve_host`, `nfm_svd_max_cols`): the bad
calls are answered with the documented codes in the documented precedence, the code objects hold exactly the
kernels the dispatch reaches (none with a private segment), and the arithmetic of the kernel -- run on the CPU
through `nfm_svd_solve_host`, the same per-record routine -- reproduces the 'svd' / 'pinv' arrays of
tests/golden/sugar.npz, the non-square cases of tests/golden/svd.npz, and leaves its sweep loop on NaN, zero and
huge records."""
import os
import re
import sys
import numpy as np
import pytest
from conftest import ROOT, GOLDEN, TOL, relerr
import _svd_ref as V

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
F32, F64 = 0, 1
PLAIN, PINV = V.PLAIN, V.PINV
SHAPES = ((2, 1), (1, 4), (8, 3), (3, 8), (7, 5), (5, 7), (8, 7))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def solve(L, dtype=F32, M=3, N=3, K=3, flags=PLAIN, rcond=1e-15, no=1, ni=1, a=4096, b=4096, out=4096, host=False):
    st = (0, 1, 1, 1)
    if host:
        return L.nfm_svd_solve_host(dtype, M, N, K, flags, rcond, no, ni, a, *st, b, *st, out, *st)
    return L.nfm_svd_solve(dtype, M, N, K, flags, rcond, no, ni, a, *st, b, *st, out, *st, None)


@pytest.mark.parametrize('host', [False, True])
def test_abi_sweep_of_nfm_svd_solve(L, host):
    """every call here is refused (or is an empty batch) before any launch: the addresses are never read"""
    def s(**kw):
        return solve(L, host=host, **kw)
    assert s(dtype=7) == EDTYPE
    assert s(ni=-1) == EINVAL and s(no=-1) == EINVAL
    assert s(no=65536) == ESIZE
    for bad in (0, 9, -1, 17):
        assert s(M=bad) == ESIZE and s(N=bad) == ESIZE and s(K=bad) == ESIZE
    assert s(flags=2) == EINVAL and s(flags=-1) == EINVAL
    assert s(rcond=-1.0) == EINVAL and s(rcond=float('nan'), flags=PINV) == EINVAL
    assert s(M=3, N=3, K=2, b=None) == EINVAL                        # identity right-hand side needs K == M
    assert s(M=3, N=5, K=5, b=None) == EINVAL and s(M=2, N=3, K=3, b=None, flags=PINV) == EINVAL
    assert s(a=None) == EINVAL and s(out=None) == EINVAL
    assert s(a=6) == EALIGN and s(b=6) == EALIGN and s(out=6) == EALIGN
    assert s(dtype=F64, a=4100) == EALIGN and s(dtype=F64, out=4100) == EALIGN
    assert s(M=3, N=5, K=3, b=None, a=None) == EINVAL and s(M=3, N=5, K=3, b=None, out=6, flags=PINV) == EALIGN
    # two errors at once: the precedence of the header
    assert s(dtype=7, N=9) == EDTYPE and s(dtype=7, ni=-1) == EDTYPE
    assert s(ni=-1, no=65536) == EINVAL and s(ni=-1, M=9) == EINVAL
    assert s(no=65536, flags=2) == ESIZE and s(M=9, flags=2) == ESIZE and s(K=0, a=None) == ESIZE
    assert s(flags=2, a=6) == EINVAL and s(M=3, K=2, b=None, a=6) == EINVAL
    assert s(dtype=F64, M=8, N=8, K=8, flags=2) == EINVAL            # the flag before the column cap
    assert s(a=None, out=6) == EINVAL and s(a=6, out=None) == EALIGN
    assert s(a=6, b=None, K=3) == EALIGN and s(b=6, out=None) == EALIGN
    # the empty batch: null pointers, no launch
    for flags in (PLAIN, PINV):
        assert s(ni=0, a=None, b=None, out=None, flags=flags) == OK
        assert s(no=0, a=None, b=None, out=None, flags=flags, dtype=F64, M=8, N=2, K=1) == OK
    assert s(ni=0, N=9, a=None, b=None, out=None) == ESIZE
    # more columns than one launch takes for this shape: the caller solves in blocks
    import torch
    from nitorch_fastmath_amd import sugar as S
    capped = 0
    for dt, code in ((torch.float32, F32), (torch.float64, F64)):
        for M in range(1, 9):
            for N in range(1, 9):
                cap = L.nfm_svd_max_cols(code, M, N)
                assert 1 <= cap <= 8 and S.svd_max_cols(dt, M, N) == cap
                assert s(dtype=code, M=M, N=N, K=cap, ni=0, a=None, b=None, out=None) == OK
                if cap < 8:
                    capped += 1
                    assert s(dtype=code, M=M, N=N, K=cap + 1) == ESIZE
    assert capped >= 1
    assert L.nfm_svd_max_cols(7, 3, 3) == EDTYPE and L.nfm_svd_max_cols(F32, 0, 3) == ESIZE
    assert L.nfm_svd_max_cols(F64, 3, 9) == ESIZE and L.nfm_svd_max_cols(F64, 9, 3) == ESIZE
    assert L.nfm_version() == 5


# ------------------------------------------------------------------------------------------------ code objects
def test_svd_kernels_in_the_census(L):
    """every (dtype, M, N, K) up to the column cap has its kernels -- the run-time-mode, contiguous and
    channel-first kinds --, every (dtype, M, N) its identity kernels, none has scratch, and nothing beyond the caps
    is compiled"""
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_svd*.o')))
    if not objs:
        pytest.skip('objects not built in this checkout (the .so alone travels to the GPU box)')
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    rows = KR.collect(objs)
    assert not [(k['kernel'], k['scratch']) for k in rows if k['scratch']]
    assert max(k['vgpr'] for k in rows) <= 512
    seen = {}
    for k in rows:
        m = re.match(r'rec_kernel<(float|double), (SvdSolveOp|SvdInvOp)<(?:float|double), (\d+), (\d+)(?:, (\d+))?>, (\d)>$',
                     k['kernel'])
        assert m, k['kernel']                       # no other kernel lives in these objects
        t, op, M, N, K, kind = m.groups()
        seen.setdefault((t, op, int(M), int(N), int(K) if K else None), set()).add(int(kind))
    want = set()
    for t, code in (('float', F32), ('double', F64)):
        for M in range(1, 9):
            for N in range(1, 9):
                want.add((t, 'SvdInvOp', M, N, None))
                for K in range(1, L.nfm_svd_max_cols(code, M, N) + 1):
                    want.add((t, 'SvdSolveOp', M, N, K))
    assert set(seen) == want, sorted(set(seen) ^ want)[:8]
    assert all(kinds >= {0, 1, 2} for kinds in seen.values())


# ------------------------------------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_entry_against_the_sugar_golden(L, dn):
    """the square 'svd' / 'pinv' arrays that tests/test_gpu_sugar.py::test_golden_parity holds the kernel to"""
    g = np.load(os.path.join(GOLDEN, 'sugar.npz'))
    most = 0
    for N in range(1, 9):
        a, b = g[f'{dn}_{N}_a'], g[f'{dn}_{N}_b']
        for name, flags in (('svd', PLAIN), ('pinv', PINV)):
            x, s1 = V.host_solve(L, a, b, flags)
            xi, s2 = V.host_solve(L, a, None, flags)
            e1, e2 = relerr(x, g[f'{dn}_{N}_lmdiv_{name}']), relerr(xi, g[f'{dn}_{N}_inv_{name}'])
            print(f'{dn} N={N} {name}: lmdiv {e1 / TOL[dn]:.3g} of the bar, inv {e2 / TOL[dn]:.3g}, sweeps {s1} {s2}')
            assert e1 <= TOL[dn] and e2 <= TOL[dn], (N, name, e1, e2)
            most = max(most, s1, s2)
    assert most < V.MAX_SWEEPS


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_entry_against_the_svd_golden(L, dn):
    """non-square lmdiv / inv / solvevec / rmdiv and the rank-7 'pinv' case, every record inside
    2 err_ref + 4 max(M, N) eps cond_2 of numpy's float64 pinv, err_ref being the golden's own error"""
    g = np.load(os.path.join(GOLDEN, 'svd.npz'))
    assert os.path.getsize(os.path.join(GOLDEN, 'svd.npz')) < 1 << 20
    worst, most = 0.0, 0

    def hold(got, ref, truth, M, N, what):
        tr, cond, den = truth
        nonlocal worst
        err, eref = V.rec_err(got, tr, den), V.rec_err(ref, tr, den)
        ex = err / (2.0 * eref + 4.0 * max(M, N) * V.EPS[dn] * cond)
        print(f'{what} {dn}: worst err / bound = {ex.max():.3g}')
        assert got.shape == ref.shape and ex.max() <= 1.0, (what, ex.max())
        worst = max(worst, ex.max())

    for M, N in SHAPES:
        def G(k):
            return g[f'{dn}_{M}x{N}_{k}']
        a, b, v, ar = G('a'), G('b'), G('v'), G('ar')
        assert a.shape == (16, M, N) and a.dtype == V.NP[dn] and b.shape == (16, M, 3)
        x, s1 = V.host_solve(L, a, b, PINV)
        hold(x, G('lmdiv'), V.truth(a, b), M, N, f'lmdiv {M}x{N}')
        xi, s2 = V.host_solve(L, a, None, PINV)
        hold(xi, G('inv'), V.truth(a, None), M, N, f'inv {M}x{N}')
        xv, s3 = V.host_solve(L, a, v[..., None], PINV)
        tv = V.truth(a, v[..., None])
        hold(xv[..., 0], G('solvevec'), (tv[0][..., 0],) + tv[1:], M, N, f'solvevec {M}x{N}')
        # rmdiv: X a = ar is a^T X^T = ar^T
        at, art = np.ascontiguousarray(a.transpose(0, 2, 1)), np.ascontiguousarray(ar.transpose(0, 2, 1))
        xr, s4 = V.host_solve(L, at, art, PINV)
        tt = V.truth(at, art)
        trr = tt[0].transpose(0, 2, 1)
        assert relerr(G('rmdiv'), trr) <= 1e-13
        hold(xr.transpose(0, 2, 1), V.torch_ref(at, art).transpose(0, 2, 1), (trr,) + tt[1:], M, N, f'rmdiv {M}x{N}')
        most = max(most, s1, s2, s3, s4)
    rc = {'f32': 1e-6, 'f64': 1e-13}[dn]
    a, b = g[f'{dn}_rank7_a'], g[f'{dn}_rank7_b']
    x, s5 = V.host_solve(L, a, b, PINV, rc)
    assert (np.linalg.matrix_rank(a.astype(np.float64)) == 7).all()
    hold(x, g[f'{dn}_rank7_lmdiv'], V.truth(a, b, rc), 8, 8, 'rank 7 pinv')
    print(f'{dn}: worst err / bound {worst:.3g}, most sweeps {max(most, s5)}')
    assert max(most, s5) < V.MAX_SWEEPS


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('shape', V.RECT_SHAPES)
def test_host_entry_rectangular_per_record(L, dn, shape):
    M, N = shape
    a, b = V.rect_case(209, M, N, 3, dn)
    x, sweeps = V.host_solve(L, a, b, PINV)
    ex = V.rect_excess(x, a, b, dn, what=f'host sweeps={sweeps}')
    assert ex.max() <= 1.0 and sweeps < V.MAX_SWEEPS


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_host_entry_pinv_threshold(L, dn):
    rc = {'f32': 1e-3, 'f64': 1e-8}[dn]
    for M, N in ((5, 5), (8, 3), (3, 8)):
        a, b = V.threshold_case(32, M, N, dn, rc, 300 + M)
        x, _ = V.host_solve(L, a, b, PINV, rc)
        assert V.rect_excess(x, a, b, dn, rc, what='threshold').max() <= 1.0


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('shape', [(2, 2), (8, 8), (8, 3), (3, 8)])
def test_host_entry_leaves_the_sweep_loop(L, dn, shape):
    """an all-NaN record, an all-zero record and a record of 1e30 entries: each returns at or below the sweep cap"""
    M, N = shape
    b = np.ones((1, M, 2), V.NP[dn])
    for fill in (np.nan, 0.0, 1e30):
        a = np.full((1, M, N), fill, V.NP[dn])
        for flags in (PLAIN, PINV):
            x, sweeps = V.host_solve(L, a, b, flags)
            assert 0 <= sweeps <= V.MAX_SWEEPS, (fill, flags, sweeps)
            if np.isnan(fill):
                assert np.isnan(x).all() and sweeps == 1
            elif fill == 0.0:
                assert sweeps == 1 and (np.array_equal(x, np.zeros_like(x)) if flags == PINV else not np.isfinite(x).any())
            elif flags == PINV:                  # rank one: the minimum-norm solution of 1e30 ones(M, N) x = ones
                assert sweeps <= 4 and np.allclose(x, 1e-30 / N, rtol=1e-5)
    a = np.random.default_rng(7).standard_normal((64, M, N)).astype(V.NP[dn])
    assert V.host_solve(L, a, np.ones((64, M, 2), V.NP[dn]), PINV)[1] <= V.MAX_SWEEPS
