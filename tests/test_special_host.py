"""Host-side checks of the special module: the golden fixture is fair (the reference's own results pass the bounds
the kernels are held to with a factor 4 to spare, and fail them by orders of magnitude where the reference is
wrong), the library exports the new symbols and validates their arguments without a GPU, the kernels' arithmetic
compiled for the CPU (`nfm_special_host_eval`) meets the fixture's bounds in both dtypes, the facade rejects what
it must, and `compat` resolves the reference's import path."""
import inspect
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _special_fixture as F


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def fx():
    return F.Fixture()


def test_fixture_is_self_consistent(fx):
    golden = os.path.dirname(F.PATH)
    assert os.path.getsize(F.PATH) <= max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden)
                                          if f.endswith('.npz') and f != 'special.npz')
    worst = {('P', 'f32'): 0.0, ('A', 'f32'): 0.0, ('A', 'f64'): 0.0}
    n = 0
    for kind, key, prm in F.cases():
        x, T = fx.x(kind, prm), fx.z['T_' + key]
        assert x.dtype == np.float32 and T.dtype == np.float64 and T.shape == x.shape
        assert fx.z['G_' + key].shape == fx.z['GB_' + key].shape == (64,)
        n += 1
        if kind != 'besseliA':
            r = F.ratio(fx.z['R32_' + key], T, fx.bound(kind, key, prm, 'f32'), 'f32')
            worst[('P', 'f32')] = max(worst[('P', 'f32')], r)
            continue
        ok = F.valid(prm['nu'], fx.z['zA'].astype(np.float64))
        assert ok.sum() >= 8 and (~ok).sum() >= 64
        for dt, ref in (('f32', fx.z['R32_' + key]), ('f64', fx.z['R64_' + key])):
            b = fx.bound(kind, key, prm, dt)
            # (the reference forms exp(f) first and overflows up to three decades early: not an error of rounding)
            use = ok & ~(np.isinf(ref) & (np.abs(T) > float(np.finfo(F.NP[dt]).max) / 1024))
            worst[('A', dt)] = max(worst[('A', dt)], F.ratio(ref[use], T[use], b[use], dt))
            # the quirk is real: outside the valid range the reference misses C by orders of magnitude
            out = F.ratio(ref[~ok], T[~ok], b[~ok], dt)
            assert out > 1e3 * fx.C(kind, dt), (key, dt, out)
    assert n == 6 + 20 + 4 + 24
    for (g, dt), w in worst.items():
        rr = float(fx.z[f'ref_ratio_{g}_{dt}'])
        C = float(fx.z[f'C_{g}_{dt}'])
        assert abs(w - rr) <= 1e-12 * rr, (g, dt, w, rr)
        assert C == 2.0 ** np.ceil(np.log2(4 * rr)) and w <= C / 4
    assert fx.z['C_P_f64'] == fx.z['C_P_f32']
    # the inputs cover both sides of the 15/4 split to the ulp, and both regimes of the general orders
    zP = fx.z['zP']
    e = np.float32(15.0 / 4.0)
    assert e in zP and np.nextafter(e, np.float32(0)) in zP and np.nextafter(e, np.float32(9)) in zP
    assert zP.min() < 2e-6 and zP.max() > 70 and fx.z['zA'].max() > 400


def test_library_exports_and_validates(L):
    bi, bib, br, brb, dg, dgb = (L.nfm_special_besseli, L.nfm_special_besseli_backward, L.nfm_special_besseli_ratio,
                                 L.nfm_special_besseli_ratio_backward, L.nfm_special_mvdigamma,
                                 L.nfm_special_mvdigamma_backward)
    assert bi(7, 0, 0.5, 1, 16, 16, None) == -2                      # dtype
    assert bi(0, 3, 0.5, 1, 16, 16, None) == -1                      # mode
    assert bi(0, -1, 0.5, 1, 16, 16, None) == -1
    assert bi(0, 0, -0.5, 1, 16, 16, None) == -1                     # nu < 0
    assert bi(0, 0, float('inf'), 1, 16, 16, None) == -1             # nu not finite
    assert bi(0, 0, float('nan'), 1, 16, 16, None) == -1
    assert bi(0, 0, 0.5, 1, None, 16, None) == -1                    # null pointer with n > 0
    assert bi(0, 0, 0.5, 1, 16, None, None) == -1
    assert bi(0, 0, 0.5, -1, 16, 16, None) == -1                     # negative count
    assert bi(0, 0, 0.5, 1, 6, 16, None) == -4                       # misaligned
    assert bi(1, 0, 0.5, 1, 16, 12, None) == -4
    assert bi(1, 2, 0.5, 0, None, None, None) == 0                   # empty
    assert bib(0, 0, 0.5, 1, 16, 16, 16, None, None) == -1
    assert bib(0, 5, 0.5, 1, 16, 16, 16, 16, None) == -1
    assert bib(3, 0, 0.5, 1, 16, 16, 16, 16, None) == -2
    assert bib(0, 0, 0.5, 1, 16, 16, 18, 16, None) == -4
    assert bib(0, 0, 0.5, 0, None, None, None, None, None) == 0
    assert br(9, 0.5, 4, 10, 1, 16, 16, None) == -2
    assert br(0, 0.5, -1, 10, 1, 16, 16, None) == -1                 # N < 0
    assert br(0, 0.5, 4, -1, 1, 16, 16, None) == -1                  # K < 0
    assert br(0, -1.0, 4, 10, 1, 16, 16, None) == -1
    assert br(0, 0.5, 9, 10, 1, 16, 16, None) == -3                  # above the compiled N
    assert br(0, 0.5, 8, 10, 1, 16, 2, None) == -4
    assert br(0, 0.5, 8, 10, 0, None, None, None) == 0
    assert brb(0, 0.5, 1, 16, 16, None, 16, None) == -1
    assert brb(1, 0.5, 1, 16, 16, 16, 4, None) == -4
    assert brb(1, 0.5, 0, None, None, None, None, None) == 0
    assert dg(0, 0, 1, 16, 16, None) == -1                           # order < 1
    assert dg(5, 1, 1, 16, 16, None) == -2
    assert dg(0, 1, 1, None, 16, None) == -1
    assert dg(0, 1, 1, 16, 6, None) == -4
    assert dg(0, 1, 0, None, None, None) == 0
    assert dgb(0, 0, 1, 16, 16, 16, None) == -1
    assert dgb(0, 2, 1, 16, None, 16, None) == -1
    assert dgb(1, 2, 0, None, None, None, None) == 0
    assert L.nfm_special_host_eval(9, 0, 0, 0.5, 0, 0, 0, None, None, None, None) == -1


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_host_build_of_the_kernel_arithmetic_meets_the_bounds(L, fx, dt):
    """nfm_special_ops.hpp is __host__ __device__: the same templates, compiled for the CPU, against every case"""
    worst = {}
    for kind, key, prm in F.cases():
        x = fx.x(kind, prm)
        gi, use = fx.grad_points(kind, key, prm, dt)
        T = fx.z['T_' + key]
        one = np.ones(len(gi))
        if kind in ('besseliP', 'besseliA'):
            got = F.host_eval(L, 'besseli', dt, x, prm['mode'], prm['nu'])
            with np.errstate(over='ignore'):
                gg = F.host_eval(L, 'besseli_bwd', dt, x[gi], prm['mode'], prm['nu'], saved=T[gi], grad=one)
        elif kind == 'ratio':
            got = F.host_eval(L, 'ratio', dt, x, 0, prm['nu'], prm['N'], prm['K'])
            gg = F.host_eval(L, 'ratio_bwd', dt, x[gi], 0, prm['nu'], saved=T[gi], grad=one)
        else:
            got = F.host_eval(L, 'mvdigamma', dt, x, prm['order'])
            gg = F.host_eval(L, 'mvdigamma_bwd', dt, x[gi], prm['order'], grad=one)
        C = fx.C(kind, dt)
        r = F.ratio(got, T, fx.bound(kind, key, prm, dt), dt)
        rg = F.ratio(gg[use], fx.z['G_' + key][use], fx.grad_bound(key, dt)[use], dt)
        worst[kind] = max(worst.get(kind, 0.0), r / C, rg / C)
        assert r <= C, (key, dt, 'forward', r, C)
        assert rg <= C, (key, dt, 'gradient', rg, C)
    print(dt, 'worst ratio / C per kind:', {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_host_special_values(L, fx, dt):
    sp = fx.z['special_x']
    for nu in F.NU_P + F.NU_A:
        for m in range(3):
            want = fx.z[f'special_bi_{F.tag(nu)}_{m}'].astype(F.NP[dt])
            with np.errstate(over='ignore'):
                got = F.host_eval(L, 'besseli', dt, sp, m, nu)
            assert F.same_pattern(got, want), (nu, m, got, want)
    for nu in F.NU_R:
        for N, K in F.NK:
            got = F.host_eval(L, 'ratio', dt, sp, 0, nu, N, K)
            assert F.same_pattern(got, fx.z[f'special_br_{F.tag(nu)}_{N}_{K}'].astype(F.NP[dt])), (nu, N, K, got)
    for order in F.ORDERS:
        x = fx.z['special_dg_x']
        want = fx.z[f'special_dg_{order}']
        got = F.host_eval(L, 'mvdigamma', dt, x, order)
        assert F.same_pattern(got, want.astype(F.NP[dt])), (order, got)
        if order > 1:       # values at order 1 only: a shifted small argument, rounded in the dtype, sits next to a pole
            continue
        assert F.special_close(got, want, order, fx.C('mvdigamma', dt), dt), (order, got, want)
        # the derivative where every trigamma is finite (small negative arguments included)
        wg = fx.z[f'special_dg_grad_{order}']
        fin = np.isfinite(wg) & (np.abs(wg) < float(np.finfo(F.NP[dt]).max))
        gg = F.host_eval(L, 'mvdigamma_bwd', dt, x[fin], order, grad=np.ones(int(fin.sum())))
        assert F.special_close(gg, wg[fin], order, fx.C('mvdigamma', dt), dt), (order, gg, wg[fin])
    # the limits of the derivative at z = 0
    z0, one = np.zeros(1), np.ones(1)
    for nu, m, want in ((1.0, 0, 0.5), (1.0, 1, 0.5), (2.5, 0, 0.0), (2.5, 1, 0.0), (0.0, 0, 0.0), (0.0, 1, -1.0), (0.0, 2, 0.0),
                        (1.0, 2, np.inf), (0.5, 2, np.inf)):
        out0 = F.host_eval(L, 'besseli', dt, z0, m, nu)
        assert F.host_eval(L, 'besseli_bwd', dt, z0, m, nu, saved=out0, grad=one)[0] == want, (nu, m)
    assert F.host_eval(L, 'ratio_bwd', dt, z0, 0, 1.5, saved=z0, grad=one)[0] == F.NP[dt](1 / 5.0)
    # the derivative is continuous into z = 0 where its limit is finite
    tiny = np.full(1, 1e-8)
    for nu, m in ((0.0, 0), (0.0, 1), (0.0, 2), (1.0, 0), (1.0, 1), (2.5, 0), (2.5, 1)):
        at0 = F.host_eval(L, 'besseli_bwd', dt, z0, m, nu, saved=F.host_eval(L, 'besseli', dt, z0, m, nu), grad=one)[0]
        near = F.host_eval(L, 'besseli_bwd', dt, tiny, m, nu, saved=F.host_eval(L, 'besseli', dt, tiny, m, nu), grad=one)[0]
        assert abs(at0 - near) <= 1e-6, (nu, m, at0, near)


def test_facade_argument_errors():
    import nitorch_fastmath_amd as N
    S = N.special
    assert S.__all__ == ['mvdigamma', 'besseli', 'besseli_ratio']
    assert list(inspect.signature(S.mvdigamma).parameters) == ['input', 'order']
    assert list(inspect.signature(S.besseli).parameters) == ['nu', 'z', 'mode']
    assert list(inspect.signature(S.besseli_ratio).parameters) == ['nu', 'X', 'N', 'K']
    assert inspect.signature(S.besseli).parameters['mode'].default is None
    assert [inspect.signature(S.besseli_ratio).parameters[k].default for k in ('N', 'K')] == [4, 10]
    assert inspect.signature(S.mvdigamma).parameters['order'].default == 1
    for call in (lambda: S.besseli(0.5, torch.ones(5)), lambda: S.besseli_ratio(0.5, torch.ones(5)),
                 lambda: S.mvdigamma(torch.ones(5)), lambda: S.besseli(0.5, 2.0), lambda: S.besseli_ratio(0, 1.0),
                 lambda: S.mvdigamma(3.0)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(ValueError):
        S.besseli(0.5, torch.ones(5), 'exp')
    with pytest.raises(ValueError):
        S.besseli(0.5, torch.ones(5), 3)
    with pytest.raises(ValueError):
        S.besseli(-1.0, torch.ones(5))
    with pytest.raises(ValueError):
        S.besseli_ratio(0.5, torch.ones(5), N=-1)
    with pytest.raises(ValueError):
        S.mvdigamma(torch.ones(5), 0)
    from nitorch_fastmath_amd._dispatch import dtype_code
    for dt in (torch.float16, torch.bfloat16, torch.complex64):
        with pytest.raises(TypeError):
            dtype_code(dt)
    # layout: dense in some order of the dims -> as is; anything else -> one contiguous copy
    t = torch.zeros(4, 5, 6)
    p = t.permute(2, 0, 1)
    assert S._dense(p) is p and S._like(p).stride() == p.stride()
    assert S._dense(t[:, ::2]).is_contiguous() and S._dense(t[:, :1]).is_contiguous()


def test_compat_resolves_special():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        importlib.import_module('nitorch_fastmath')
        from nitorch_fastmath.special import besseli, besseli_ratio, mvdigamma
        import nitorch_fastmath_amd as N
        assert besseli is N.special.besseli and besseli_ratio is N.special.besseli_ratio
        assert mvdigamma is N.special.mvdigamma
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)
