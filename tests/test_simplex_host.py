"""Host-side checks of the simplex module: the golden fixture is fair (the reference's own float32 result
passes the bounds the kernels are held to), the library exports the new symbols and validates their
arguments without a GPU, the facade rejects what it must, and `compat` resolves the reference's import path."""
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT
import _simplex_fixture as F


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


def test_fixture_is_self_consistent():
    fx = F.Fixture()
    assert os.path.getsize(F.PATH) <= os.path.getsize(os.path.join(os.path.dirname(F.PATH), 'lie.npz'))
    worst, n = 0.0, 0
    for fn, K, inner, dt, imp, idx in F.cases():
        x = fx.x(fn, K, inner, dt, imp)
        truth = fx.truth(fn, K, inner, imp, idx, exact_added=False)     # the reference against itself
        ref = fx.ref(fn, K, inner, dt, imp, idx)
        assert ref.shape == truth.shape == (x.shape[0], K + imp[0] - imp[1] if fn != 'logsumexp' else 1, x.shape[2])
        assert np.array_equal(np.isnan(ref), np.isnan(truth)) or dt == 'f32'
        worst = max(worst, F.ratio(ref, truth, F.bound(fn, x, truth, imp, idx, dt, slack=True)))
        n += 1
    assert n > 1000
    # C follows from the reference's own float32 error: next power of two at or above 4 x its worst ratio
    assert abs(worst - fx.ref_ratio) <= 1e-12 * worst
    assert fx.C == 2.0 ** np.ceil(np.log2(4 * fx.ref_ratio)) and worst <= fx.C / 4
    # the cancellation-free truth of the added class agrees with the reference's 1 - sum(p) to the latter's error
    for K, inner in ((3, 7), (16, 64), (40, 1)):
        a = fx.truth('softmax', K, inner, (True, False), 0)[:, 0]
        b = fx.truth('softmax', K, inner, (True, False), 0, exact_added=False)[:, 0]
        assert np.abs(a - b).max() <= 4 * F.EPS['f64'] * (K + 1)
    # the inputs are fair: float32 exp underflows in some classes, and not everywhere
    p = fx.ref('softmax', 40, 64, 'f32', (False, False), 0)
    assert (p == 0).any() and (p > 0.01).any()


def test_library_exports_and_validates(L):
    f, b = L.nfm_simplex_forward, L.nfm_simplex_backward
    assert f(7, 0, 0, 0, 1, 3, 1, 16, 16, None, None) == -2          # dtype
    assert f(0, 9, 0, 0, 1, 3, 1, 16, 16, None, None) == -1          # op
    assert f(0, 4, 0, 0, 1, 3, 1, 16, 16, None, None) == -1          # a backward op
    assert f(0, 0, 4, 0, 1, 3, 1, 16, 16, None, None) == -1          # flags
    assert f(0, 0, 0, 3, 1, 3, 1, 16, 16, None, None) == -1          # index out of the K' classes
    assert f(0, 0, 1, 3, 0, 3, 1, None, None, None, None) == 0       # ... inside them with a hidden class; empty
    assert f(0, 0, 0, 0, 1, 0, 1, 16, 16, None, None) == -1          # no classes
    assert f(0, 0, 2, 0, 1, 1, 1, 16, 16, None, None) == -1          # the only class dropped
    assert f(0, 0, 0, 0, 1, 49, 1, 16, 16, None, None) == -3         # above NFM_SIMPLEX_MAX_K
    assert f(0, 0, 0, 0, 1, 3, 1, 6, 16, None, None) == -4           # misaligned
    assert f(0, 0, 0, 0, 1, 3, 1, 16, None, None, None) == -1        # no output
    assert f(0, 2, 0, 0, 1, 3, 1, 16, None, None, None) == -1        # logsumexp without lse
    assert f(0, 1, 0, 0, 1, 3, 1, 16, 16, 16, None) == -1            # lse beside log_softmax
    assert f(1, 0, 0, 0, 5, 3, 0, None, None, None, None) == 0       # empty
    assert b(0, 0, 0, 0, 1, 3, 1, 16, 16, 16, None) == -1            # a forward op
    assert b(0, 4, 0, 0, 1, 3, 1, 16, None, 16, None) == -1
    assert b(1, 5, 1, 3, 0, 3, 7, None, None, None, None) == 0


def test_facade_argument_errors():
    import nitorch_fastmath_amd as N
    S = N.simplex
    assert S.__all__ == ['logsumexp', 'softmax', 'log_softmax', 'logit', 'softmax_lse']
    for fn in (S.softmax, S.log_softmax, S.logit, S.logsumexp, S.softmax_lse):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(torch.ones(5, 3))
    import inspect
    assert list(inspect.signature(S.logsumexp).parameters) == ['input', 'dim', 'keepdim', 'implicit']
    assert list(inspect.signature(S.softmax).parameters) == ['input', 'dim', 'implicit', 'implicit_index']
    assert list(inspect.signature(S.log_softmax).parameters) == ['input', 'dim', 'implicit', 'implicit_index']
    assert list(inspect.signature(S.logit).parameters) == ['input', 'dim', 'implicit', 'implicit_index']
    assert list(inspect.signature(S.softmax_lse).parameters) == ['input', 'dim', 'weights', 'implicit']
    assert S._pair(True) == (True, True) and S._pair((True, False)) == (True, False)
    assert S._index(-1, 4) == 3 and S._index(2, 4) == 2
    for bad in (4, -5):
        with pytest.raises(IndexError):
            S._index(bad, 4)
    with pytest.raises(ValueError):
        S._pair((True, False, True))
    with pytest.raises(TypeError):
        S.logsumexp(torch.ones(2, 3), 1, False, (True, False))
    from nitorch_fastmath_amd._dispatch import dtype_code
    for dt in (torch.float16, torch.bfloat16, torch.complex64):
        with pytest.raises(TypeError):
            dtype_code(dt)


def test_compat_resolves_simplex():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        importlib.import_module('nitorch_fastmath')
        from nitorch_fastmath.simplex import softmax, log_softmax, logsumexp, logit, softmax_lse  # noqa: F401
        import nitorch_fastmath_amd as N
        assert softmax is N.simplex.softmax
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)
