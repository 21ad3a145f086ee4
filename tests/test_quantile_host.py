"""CPU-side checks of reduce.quantile / nanquantile: the C ABI of nfm_reduce_quantile answers without a GPU,
the kernels' rank routine (run on the host by nfm_reduce_quantile_plan_host) agrees with the model of
tests/_quantile_ref.py, and the facade's surface: signatures, q validation, result shapes, q blocking."""
import ctypes
import inspect
import os
import numpy as np
import pytest
import torch
from conftest import ROOT
import _quantile_ref as QR

OK, EINVAL, EDTYPE, ESIZE = 0, -1, -2, -3
F32, F64 = 0, 1
LINEAR, LOWER, HIGHER, NEAREST, MIDPOINT = range(5)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


def quant(L, dtype=F32, omitnan=0, interp=LINEAR, rows=4, red=100, q=(0.5,), nq=None, x=4096, ws=None, wsn=0,
          val=8192, pos=None):
    """nfm_reduce_quantile on made-up addresses: only for calls that are refused (or empty) before any launch"""
    qarr = None if q is None else (ctypes.c_double * max(len(q), 1))(*q)
    return L.nfm_reduce_quantile(dtype, omitnan, interp, rows, red, len(q) if nq is None else nq, qarr, x, ws, wsn, val,
                                 pos, None)


def test_abi_sweep_of_nfm_reduce_quantile(L):
    """every call here is refused (or is an empty batch) before any launch: the addresses are never read"""
    def s(**kw):
        return quant(L, **kw)
    cap = L.nfm_reduce_quantile_max_q()
    assert cap >= 4
    # every refusal code
    assert s(dtype=7) == EDTYPE and s(dtype=-1) == EDTYPE
    assert s(rows=-1) == EINVAL and s(red=-1) == EINVAL
    assert s(nq=0) == EINVAL and s(nq=-3) == EINVAL
    assert s(interp=5) == EINVAL and s(interp=-1) == EINVAL
    assert s(q=(1.5,)) == EINVAL and s(q=(-1e-9,)) == EINVAL and s(q=(float('nan'),)) == EINVAL
    assert s(q=(0.5, 0.25, 2.0)) == EINVAL                     # any entry
    assert s(q=None, nq=1) == EINVAL and s(x=None) == EINVAL and s(val=None) == EINVAL
    assert s(red=0) == EINVAL
    assert s(q=(0.5,) * (cap + 1)) == ESIZE
    assert s(rows=65536, red=1025, ws=64, wsn=1 << 40) == ESIZE  # the long-row form: grid.y
    need = L.nfm_reduce_quantile_workspace_bytes(4, 2000, 1)
    assert need > 0
    assert s(red=2000) == EINVAL                               # no workspace: the code nfm_reduce_median uses
    assert s(red=2000, ws=64, wsn=need - 1) == EINVAL
    assert L.nfm_reduce_median(F32, 0, 4, 2000, 4096, 64, 8, 8192, None, None) == EINVAL
    # two errors at once: the precedence of the header
    assert s(dtype=7, rows=-1) == EDTYPE and s(dtype=7, nq=cap + 1) == EDTYPE and s(dtype=7, q=(2.0,)) == EDTYPE
    assert s(rows=-1, q=(0.5,) * (cap + 1)) == EINVAL and s(interp=9, q=(0.5,) * (cap + 1)) == EINVAL
    assert s(q=(2.0,) * (cap + 1)) == ESIZE and s(q=None, nq=cap + 1) == ESIZE      # the cap before q is read
    assert s(q=(2.0,), x=None, rows=0) == EINVAL               # a bad q before the empty batch
    assert s(q=(2.0,), rows=65536, red=1025) == EINVAL and s(x=None, rows=65536, red=1025) == EINVAL
    assert s(rows=65536, red=1025, ws=None) == ESIZE           # grid.y before the workspace
    # the empty batch: null pointers, no launch
    assert s(rows=0, x=None, val=None) == OK and s(rows=0, red=0, x=None, val=None, dtype=F64) == OK
    assert s(rows=0, red=5000, x=None, val=None, ws=None) == OK
    assert s(rows=0, nq=0, x=None, val=None) == EINVAL
    # nq at the cap and one beyond
    assert s(q=(0.5,) * cap, rows=0, x=None, val=None) == OK
    assert s(q=(0.5,) * (cap + 1), rows=0, x=None, val=None) == ESIZE
    # the workspace: none for rows in registers, growing with nq beyond
    W = L.nfm_reduce_quantile_workspace_bytes
    assert W(100, 1, 3) == 0 and W(100, 32, cap) == 0 and W(100, 1024, cap) == 0 and W(0, 5000, 1) == 0
    sizes = [W(7, 1025, n) for n in range(1, cap + 1)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert W(14, 1025, 2) == 2 * W(7, 1025, 2)
    assert L.nfm_version() == 5


COUNTS = (1, 2, 3, 4, 7, 2 ** 24 + 1, 2 ** 33 + 5)
QS = (0.0, 1.0, 0.5, 0.25, 1 / 3, 2 / 3, 1e-9, 1 - 2.0 ** -53)


def plan_host(L, q, count, interp):
    lo, hi, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
    assert L.nfm_reduce_quantile_plan_host(q, count, interp, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(w)) == OK
    return lo.value, hi.value, w.value


def test_rank_routine_against_the_model(L):
    for code, name in enumerate(QR.INTERPS):
        assert name == ('linear', 'lower', 'higher', 'nearest', 'midpoint')[code]
        for count in COUNTS + (6,):
            for q in QS + (0.3,):
                got = plan_host(L, q, count, code)
                assert got == QR.plan(q, count, name), (name, count, q, got)
                assert got[0] <= got[1] <= count - 1 and 0.0 <= got[2] < 1.0
    # half to even, as numpy and torch: count = 6, q = 0.5 -> p = 2.5 -> rank 2; q = 0.3 -> p = 1.5 -> rank 2
    assert plan_host(L, 0.5, 6, NEAREST) == (2, 2, 0.0)
    assert plan_host(L, 0.3, 6, NEAREST) == (2, 2, 0.0)
    assert plan_host(L, 0.7, 6, NEAREST) == (4, 4, 0.0)            # p = 3.5 -> 4
    assert plan_host(L, 0.5, 6, LINEAR) == (2, 3, 0.5) and plan_host(L, 0.5, 6, MIDPOINT) == (2, 3, 0.5)
    assert plan_host(L, 0.5, 6, LOWER) == (2, 2, 0.0) and plan_host(L, 0.5, 6, HIGHER) == (3, 3, 0.0)
    assert plan_host(L, 1 - 2.0 ** -53, 2 ** 33 + 5, LOWER)[0] == 2 ** 33 + 3
    assert plan_host(L, 1.0, 2 ** 33 + 5, LINEAR) == (2 ** 33 + 4, 2 ** 33 + 4, 0.0)
    # refusals
    z = ctypes.c_uint64()
    w = ctypes.c_double()
    P = L.nfm_reduce_quantile_plan_host
    assert P(0.5, 0, 0, ctypes.byref(z), ctypes.byref(z), ctypes.byref(w)) == EINVAL
    assert P(1.5, 3, 0, ctypes.byref(z), ctypes.byref(z), ctypes.byref(w)) == EINVAL
    assert P(float('nan'), 3, 0, ctypes.byref(z), ctypes.byref(z), ctypes.byref(w)) == EINVAL
    assert P(0.5, 3, 5, ctypes.byref(z), ctypes.byref(z), ctypes.byref(w)) == EINVAL
    assert P(0.5, 3, 0, None, ctypes.byref(z), ctypes.byref(w)) == EINVAL
    assert P(0.5, 3, 0, ctypes.byref(z), ctypes.byref(z), None) == EINVAL


def test_model_on_known_values():
    """the model itself, on cases worked by hand"""
    x = np.array([[4.0, 1.0, 3.0, 2.0]])
    m = QR.quantiles(x, [0.0, 0.5, 1.0, 0.25], False)
    assert [float(v[0]) for v in m['linear'][0]] == [1.0, 2.5, 4.0, 1.75]
    assert [float(v[0]) for v in m['lower'][0]] == [1.0, 2.0, 4.0, 1.0]
    assert [float(v[0]) for v in m['higher'][0]] == [1.0, 3.0, 4.0, 2.0]
    assert [float(v[0]) for v in m['nearest'][0]] == [1.0, 3.0, 4.0, 2.0]       # p = 1.5 -> rank 2; p = 0.75 -> rank 1
    assert [float(v[0]) for v in m['midpoint'][0]] == [1.0, 2.5, 4.0, 1.5]
    inf = float('inf')
    y = np.array([[inf, inf, 1.0, float('nan')]])
    assert np.isnan(QR.quantiles(y, [0.5], False)['linear'][0][0][0])
    assert QR.quantiles(y, [0.75], True)['linear'][0][0][0] == inf                  # equal infinities: that infinity
    assert QR.quantiles(y, [0.2], True)['linear'][0][0][0] == inf                   # w < 0.5: 1 + 0.4 * inf
    assert np.isnan(QR.quantiles(y, [0.3], True)['linear'][0][0][0])                # w >= 0.5: inf - inf * 0.4 (IEEE)
    assert np.isnan(QR.quantiles(np.full((1, 3), np.nan), [0.5], True)['lower'][0][0][0])


# ------------------------------------------------------------------------------------------------ facade
def test_signatures_and_all():
    from nitorch_fastmath_amd import reduce as R

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(R.quantile) == [('input', E), ('q', E), ('dim', None), ('keepdim', False), ('omitnan', False),
                               ('inplace', False), ('interpolation', 'linear'), ('out', None)]
    assert sig(R.nanquantile) == [('input', E), ('q', E), ('dim', None), ('keepdim', False), ('inplace', False),
                                  ('interpolation', 'linear'), ('out', None)]
    assert 'quantile' in R.__all__ and 'nanquantile' in R.__all__
    assert R.__all__[:5] == ['min', 'max', 'nanmin', 'nanmax', 'median']


def test_cpu_tensors_are_refused():
    from nitorch_fastmath_amd import reduce as R
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        R.quantile(torch.ones(4, 5), 0.5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        R.nanquantile(torch.ones(4, 5), [0.1, 0.9], dim=1)


@pytest.fixture
def calls(monkeypatch, L):
    """`reduce._quantile_call` replaced by a recorder: nothing runs (CPU tensors never reach a kernel)"""
    from nitorch_fastmath_amd import reduce as R
    seen = []

    def record(dev, code, omitnan, interp, x, qb, val, pos):
        assert val.shape == (len(qb), x.shape[0]) and val.is_contiguous() and x.is_contiguous()
        seen.append((code, bool(omitnan), interp, tuple(x.shape), list(qb), pos is not None))
        val.zero_()
        if pos is not None:
            pos.zero_()
    monkeypatch.setattr(R, '_quantile_call', record)
    monkeypatch.setattr(R, 'require_gpu', lambda *tensors: tensors[0].device)
    return seen


def test_bad_q_and_interpolation(calls):
    from nitorch_fastmath_amd import reduce as R
    x = torch.zeros(3, 5)
    for q in (1.5, -0.1, float('nan'), [], [0.5, 1.0000001], torch.tensor([0.2, float('nan')]), torch.zeros(0),
              torch.zeros(2, 2)):
        with pytest.raises(ValueError):
            R.quantile(x, q)
    for bad in ('cubic', 'Linear', None, 0):
        with pytest.raises(ValueError):
            R.quantile(x, 0.5, interpolation=bad)
    with pytest.raises(IndexError):
        R.quantile(torch.zeros(3, 0), 0.5, dim=1)
    with pytest.raises(IndexError):
        R.quantile(x, 0.5, dim=2)
    with pytest.raises(TypeError):
        R.quantile(x.half(), 0.5)
    with pytest.raises(RuntimeError, match='out='):
        R.quantile(x.clone().requires_grad_(), 0.5, out=torch.zeros(()))
    assert calls == []


def test_result_shapes_and_q_blocking(calls, L):
    from nitorch_fastmath_amd import reduce as R
    cap = L.nfm_reduce_quantile_max_q()
    x = torch.zeros(5, 7, 11, dtype=torch.float64)
    assert R.quantile(x, 0.5).shape == () and R.quantile(x, [0.5]).shape == (1,)
    assert R.quantile(x, 0.5, keepdim=True).shape == (1, 1, 1)
    assert R.quantile(x, [0.1, 0.2, 0.3], keepdim=True).shape == (3, 1, 1, 1)
    assert R.quantile(x, 0.5, dim=1).shape == (5, 11) and R.quantile(x, (0.1, 0.9), dim=1).shape == (2, 5, 11)
    assert R.quantile(x, torch.tensor([0.1, 0.9]), dim=[0, 2]).shape == (2, 7)
    assert R.quantile(x, torch.tensor(0.3), dim=[0, 2], keepdim=True).shape == (1, 7, 1)
    assert R.nanquantile(x, np.array([0.1, 0.9, 1.0]), dim=-1, keepdim=True).shape == (3, 5, 7, 1)
    assert calls[0] == (F64, False, LINEAR, (1, 385), [0.5], False)
    assert calls[-1] == (F64, True, LINEAR, (35, 11), [0.1, 0.9, 1.0], False)
    out = torch.empty(0, dtype=torch.float64)
    assert R.quantile(x, [0.5, 0.6], dim=0, out=out) is out and out.shape == (2, 7, 11)
    # interpolation codes as the header numbers them
    del calls[:]
    for name in QR.INTERPS:
        R.quantile(x, 0.5, dim=2, interpolation=name)
    assert [c[2] for c in calls] == [LINEAR, LOWER, HIGHER, NEAREST, MIDPOINT]
    # a q list longer than the cap runs in blocks of the cap, in order
    del calls[:]
    qs = [k / (2 * cap + 3) for k in range(2 * cap + 3)]
    assert R.quantile(x.float(), qs, dim=1).shape == (2 * cap + 3, 5, 11)
    assert [c[4] for c in calls] == [qs[:cap], qs[cap:2 * cap], qs[2 * cap:]] and calls[0][0] == F32
    # long rows are split so that one call's workspace stays within the budget
    del calls[:]
    W = L.nfm_reduce_quantile_workspace_bytes
    step = R._QUANTILE_WS_BUDGET // W(1, 1025, cap)
    assert 1 <= step < 65535
    y = torch.zeros(step + 2, 1025)
    R.quantile(y, [0.5] * cap, dim=1)
    assert [c[3] for c in calls] == [(step, 1025), (2, 1025)]
    assert all(W(c[3][0], 1025, cap) <= R._QUANTILE_WS_BUDGET for c in calls)
    # with a gradient the kernel is asked for the positions
    del calls[:]
    xg = torch.arange(15.0).reshape(3, 5).requires_grad_()
    R.quantile(xg, 0.5, dim=1).sum().backward()        # positions (0, 0) from the recorder: the first column
    assert len(calls) == 1 and calls[0][5] is True
    assert torch.equal(xg.grad, torch.tensor([1.0, 0, 0, 0, 0]).expand(3, 5))
