"""CPU-side checks of the tall least-squares solves (`nfm_lstsq_solve`, `nfm_lstsq_solve_host`,
`nfm_lstsq_max_cols`): the bad calls are answered with the documented codes in the documented precedence, the code
objects hold exactly the kernels the dispatch reaches (none with a private segment), and the arithmetic of the
kernel -- run on the CPU through `nfm_lstsq_solve_host`, the same per-record routine -- stays inside
2 err_ref + 4 N eps cond_2 of numpy's float64 `pinv(a, rcond) @ b` for every record (tests/_lstsq_ref.py) on graded
records from 9 x 1 to 257 x 3, over the whole exponent range, at the rcond cut, on exactly rank-deficient records
and on the reference's own results (tests/golden/lstsq.npz)."""
import os
import re
import sys
import numpy as np
import pytest
from conftest import ROOT, GOLDEN
import _solver_ref as R
import _svd_ref as V
import _lstsq_ref as Q

OK, EINVAL, EDTYPE, ESIZE, EALIGN = 0, -1, -2, -3, -4
F32, F64 = 0, 1
DNS = ['f32', 'f64']


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def solve(L, dtype=F32, M=12, N=3, K=2, rcond=1e-15, no=1, ni=1, a=4096, b=4096, out=4096, host=False):
    st = (0, 1, 1, 1)
    if host:
        return L.nfm_lstsq_solve_host(dtype, M, N, K, rcond, no, ni, a, *st, b, *st, out, *st)
    return L.nfm_lstsq_solve(dtype, M, N, K, rcond, no, ni, a, *st, b, *st, out, *st, None)


@pytest.mark.parametrize('host', [False, True])
def test_abi_sweep_of_nfm_lstsq_solve(L, host):
    """every call here is refused (or is an empty batch) before any launch: the addresses are never read"""
    def s(**kw):
        return solve(L, host=host, **kw)
    assert s(dtype=7) == EDTYPE
    assert s(ni=-1) == EINVAL and s(no=-1) == EINVAL
    assert s(no=65536) == ESIZE
    for bad in (0, 9, -1, 17):
        assert s(N=bad, M=20) == ESIZE and s(K=bad) == ESIZE
    assert s(M=2, N=3) == ESIZE and s(M=0, N=1) == ESIZE and s(M=-5) == ESIZE      # M = N - 1 and below
    assert s(M=4097) == ESIZE and s(M=4096, ni=0, a=None, b=None, out=None) == OK
    assert s(M=3, N=3, ni=0, a=None, b=None, out=None) == OK                      # M = N is a system
    assert s(rcond=-1.0) == EINVAL and s(rcond=float('nan')) == EINVAL
    assert s(a=None) == EINVAL and s(b=None) == EINVAL and s(out=None) == EINVAL
    assert s(a=6) == EALIGN and s(b=6) == EALIGN and s(out=6) == EALIGN
    assert s(dtype=F64, a=4100) == EALIGN and s(dtype=F64, out=4100) == EALIGN
    # two errors at once: the precedence of the header
    assert s(dtype=7, N=9) == EDTYPE and s(dtype=7, ni=-1) == EDTYPE
    assert s(ni=-1, no=65536) == EINVAL and s(ni=-1, N=9) == EINVAL
    assert s(no=65536, rcond=-1.0) == ESIZE and s(N=9, M=20, rcond=-1.0) == ESIZE and s(K=0, a=None) == ESIZE
    assert s(M=4097, rcond=-1.0) == ESIZE and s(M=2, rcond=float('nan')) == ESIZE   # the rows before rcond
    assert s(rcond=-1.0, a=6) == EINVAL and s(rcond=-1.0, a=None) == EINVAL
    assert s(a=None, out=6) == EINVAL and s(a=6, out=None) == EALIGN
    assert s(a=6, b=None) == EALIGN and s(b=6, out=None) == EALIGN and s(b=None, out=6) == EINVAL
    # the empty batch: null pointers, no launch
    assert s(ni=0, a=None, b=None, out=None) == OK
    assert s(no=0, a=None, b=None, out=None, dtype=F64, M=4096, N=8, K=1) == OK
    assert s(ni=0, N=9, M=20, a=None, b=None, out=None) == ESIZE
    assert s(ni=0, M=2, N=3, a=None, b=None, out=None) == ESIZE
    assert s(ni=0, rcond=-1.0, a=None, b=None, out=None) == EINVAL
    # more columns than one launch takes at this N: the caller solves in blocks
    import torch
    from nitorch_fastmath_amd import sugar as S
    capped = 0
    for dt, code in ((torch.float32, F32), (torch.float64, F64)):
        for N in range(1, 9):
            cap = L.nfm_lstsq_max_cols(code, N)
            assert 1 <= cap <= min(8, L.nfm_svd_max_cols(code, N, N)) and S.lstsq_max_cols(dt, N) == cap
            assert s(dtype=code, M=40, N=N, K=cap, ni=0, a=None, b=None, out=None) == OK
            assert s(dtype=code, M=40, N=N, K=cap + 1) == ESIZE
            if cap < 8:
                capped += 1
                assert s(dtype=code, M=40, N=N, K=cap + 1, rcond=-1.0) == EINVAL   # rcond before the column cap
    assert capped >= 1
    assert L.nfm_lstsq_max_cols(7, 3) == EDTYPE and L.nfm_lstsq_max_cols(F32, 0) == ESIZE
    assert L.nfm_lstsq_max_cols(F64, 9) == ESIZE and L.nfm_lstsq_max_cols(-1, 9) == EDTYPE
    assert L.nfm_version() == 5


# ------------------------------------------------------------------------------------------------ code objects
def test_lstsq_kernels_in_the_census(L):
    """every (dtype, N, K) up to the column cap has its two kernels -- the LDS-staged contiguous one and the
    per-lane one --, none has scratch, and nothing beyond the caps is compiled"""
    import glob
    objs = sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_lstsq*.o')))
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
        m = re.match(r'lstsq_(tile|lane)_kernel<(float|double), (\d+), (\d+)>$', k['kernel'])
        assert m, k['kernel']                       # no other kernel lives in these objects
        kind, t, N, K = m.groups()
        seen.setdefault((t, int(N), int(K)), set()).add(kind)
    want = set()
    for t, code in (('float', F32), ('double', F64)):
        for N in range(1, 9):
            for K in range(1, L.nfm_lstsq_max_cols(code, N) + 1):
                want.add((t, N, K))
    assert set(seen) == want, sorted(set(seen) ^ want)[:8]
    assert all(kinds == {'tile', 'lane'} for kinds in seen.values())


# ------------------------------------------------------------------------------------------------ the arithmetic
def hold(L, a, b, dn, rcond=1e-15, what='', ref=None):
    x, sweeps = Q.host_solve(L, a, b, rcond)
    ex = Q.excess(x, a, b, dn, rcond, what=f'host {what} sweeps={sweeps}', ref=ref)
    assert x.shape == (len(a), a.shape[-1], b.shape[-1]) and x.dtype == a.dtype
    assert ex.max() <= 1.0, (what, ex.max())
    assert sweeps < Q.MAX_SWEEPS
    return x


@pytest.mark.parametrize('dn', DNS)
@pytest.mark.parametrize('shape', Q.SHAPES)
def test_host_entry_per_record(L, dn, shape):
    """graded records with per-record exponents in +-6; M = N + 1 and M = 17 (one row past a row block) are the
    cases that matter"""
    M, N, K = shape
    K = L.nfm_lstsq_max_cols(Q.CODE[dn], N) if K is None else K
    a, b = Q.tall_case(65, M, N, K, dn, 4000 + 10 * M + N)
    hold(L, a, b, dn, what='graded')


@pytest.mark.parametrize('dn', DNS)
def test_host_entry_whole_exponent_range(L, dn):
    """33 x 6 records times 2^k, k over +-90 (float32) / +-900 (float64): naive squares overflow and underflow"""
    kmax = {'f32': 90, 'f64': 900}[dn]
    k = R.pow2_scales(65, kmax, 77)
    assert k.min() == -kmax and k.max() == kmax
    a, b = Q.tall_case(65, 33, 6, 1, dn, 4100, exps=tuple(int(v) for v in k))
    x = hold(L, a, b, dn, what=f'2^+-{kmax}')
    assert np.isfinite(x).all()


@pytest.mark.parametrize('dn', DNS)
def test_host_entry_cut(L, dn):
    """the smallest singular value at rcond sigma_max 10^(+-1.5): odd records drop it, even ones keep it; and
    records of rank exactly 5"""
    rc = {'f32': 1e-4, 'f64': 1e-10}[dn]
    a, b = V.threshold_case(64, 33, 6, dn, rc, 4200)
    hold(L, a, b, dn, rc, what='threshold')
    rc = {'f32': 1e-6, 'f64': 1e-13}[dn]
    a, b = Q.rank5_case(32, dn, 4300)
    hold(L, a, b, dn, rc, what='rank 5')


@pytest.mark.parametrize('dn', DNS)
def test_host_entry_agrees_with_the_jacobi_path(L, dn):
    """a 33 x 6 record whose rows 8.. are zero is the 8 x 6 system of its first rows (nfm_svd_solve_host)"""
    a8, b8 = Q.tall_case(32, 8, 6, 2, dn, 4400)
    a = np.zeros((32, 33, 6), Q.NP[dn])
    b = np.random.default_rng(4401).standard_normal((32, 33, 2)).astype(Q.NP[dn])
    a[:, :8], b[:, :8] = a8, b8
    x = hold(L, a, b, dn, what='zero rows')
    x8, _ = V.host_solve(L, a8, b8, V.PINV)
    assert Q.excess(x, a8, b8, dn, what='against 8 x 6', ref=x8).max() <= 1.0
    assert Q.excess(x8, a8, b8, dn, what='8 x 6 against it', ref=x).max() <= 1.0


@pytest.mark.parametrize('dn', DNS)
def test_host_entry_degenerate(L, dn):
    """an all-zero record gives X = 0; a NaN in one record of three leaves the other two bit-identical"""
    b = np.ones((1, 33, 2), Q.NP[dn])
    x, sweeps = Q.host_solve(L, np.zeros((1, 33, 6), Q.NP[dn]), b)
    assert np.array_equal(x, np.zeros_like(x)) and sweeps < Q.MAX_SWEEPS
    a, b = Q.tall_case(3, 33, 6, 2, dn, 4500)
    clean, s0 = Q.host_solve(L, a, b)
    for where in ((1, 0, 0), (1, 32, 5), (1, 17, 3)):
        bad = a.copy()
        bad[where] = np.nan
        got, s1 = Q.host_solve(L, bad, b)
        assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], clean[[0, 2]]), where
        assert s1 < Q.MAX_SWEEPS
    bb = b.copy()
    bb[1, 20, 1] = np.nan
    got, s2 = Q.host_solve(L, a, bb)
    assert np.isnan(got[1, :, 1]).all() and np.array_equal(got[[0, 2]], clean[[0, 2]]) and s2 < Q.MAX_SWEEPS
    inf = a.copy()
    inf[1, 4, 2] = np.inf
    got, s3 = Q.host_solve(L, inf, b)
    assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], clean[[0, 2]]) and s3 < Q.MAX_SWEEPS
    # strides are honoured: a stored transposed, one b for every record
    at = np.ascontiguousarray(a.transpose(0, 2, 1))
    out = np.empty((3, 6, 2), Q.NP[dn])
    e = a.itemsize
    rc = L.nfm_lstsq_solve_host(Q.CODE[dn], 33, 6, 2, 1e-15, 1, 3, at.ctypes.data, 0, at.strides[0] // e, 1, 33,
                                b.ctypes.data, 0, 0, 2, 1, out.ctypes.data, 0, 12, 2, 1)
    assert rc >= 0 and np.array_equal(out, Q.host_solve(L, a, np.broadcast_to(b[0], b.shape))[0])


@pytest.mark.parametrize('dn', DNS)
def test_host_entry_against_the_golden(L, dn):
    """the reference's own lmdiv results (tests/golden/lstsq.npz) as err_ref"""
    path = os.path.join(GOLDEN, 'lstsq.npz')
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path)
    for M, N in ((12, 3), (33, 6), (64, 8)):
        a, b, ref = (g[f'{dn}_{M}x{N}_{k}'] for k in ('a', 'b', 'lmdiv'))
        assert a.shape == (16, M, N) and a.dtype == Q.NP[dn] and b.shape == (16, M, 2) and ref.shape == (16, N, 2)
        hold(L, a, b, dn, what='golden', ref=ref)
