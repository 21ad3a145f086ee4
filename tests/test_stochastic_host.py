"""CPU-side checks of the stochastic module: the Philox known answers (the numpy model AND the library's own
generator), argument validation of the three entry points without a GPU, the facade's refusals, the
reference's signatures, the compat import paths and the host-side maximum-entropy fit of vbald."""
import ctypes
import importlib
import inspect
import json
import os
import sys
import numpy as np
import pytest
import torch
from conftest import ROOT, GOLDEN
import _stochastic_ref as R

# Philox4x32-10: counter, key -> output (Random123's known-answer vectors)
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as G
    if not os.path.exists(os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')):
        G.build()
    from nitorch_fastmath_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers_model(ctr, key, want):
    assert [int(w[0]) for w in R.philox4x32_10(ctr, key)] == want


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers_library(L, ctr, key, want):
    c, k, out = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    assert L.nfm_stoch_philox_host(c, k, out) == 0
    assert list(out) == want


def test_model_streams_are_functions_of_the_element_index():
    # a range split anywhere, or started anywhere, gives the same elements
    for fn in (R.rademacher, R.gaussian):
        whole = fn(12345, 77, 1000)
        assert np.array_equal(np.concatenate([fn(12345, 77, 333), fn(12345, 410, 667)]), whole)
    r = R.rademacher(7, 0, 1 << 16)
    assert set(np.unique(r)) == {-1.0, 1.0} and abs(r.mean()) < 4 / 256
    g = R.gaussian(7, 0, 1 << 16)
    assert abs(g.mean()) < 4 / 256 and abs(g.var() - 1) < 0.03


def test_argument_validation_without_gpu(L):
    EINVAL, EDTYPE, ESIZE, EALIGN, EWORKSPACE = -1, -2, -3, -4, -5
    p8 = (ctypes.c_void_p * 8)(*([64] * 8))          # never dereferenced: every call below is rejected before a launch
    # fill: dtype, kind, negative n / offset, null output, alignment; an empty range is a success without a launch
    assert L.nfm_stoch_fill(7, 0, 1, 0, 10, 64, None) == EDTYPE
    assert L.nfm_stoch_fill(0, 2, 1, 0, 10, 64, None) == EINVAL
    assert L.nfm_stoch_fill(0, 0, 1, 0, -1, 64, None) == EINVAL
    assert L.nfm_stoch_fill(0, 0, 1, -5, 10, 64, None) == EINVAL
    assert L.nfm_stoch_fill(0, 0, 1, 0, 10, None, None) == EINVAL
    assert L.nfm_stoch_fill(1, 1, 1, 0, 10, 68, None) == EALIGN
    assert L.nfm_stoch_fill(0, 0, 1, 0, 0, None, None) == 0
    # gram: p or q of 0 or 9, dtype, n < 0, workspace
    for p, q in [(0, 1), (9, 1), (1, 0), (1, 9)]:
        assert L.nfm_stoch_gram(0, p, q, 10, p8, p8, 64, 1 << 30, 64, 0, None) == ESIZE
        assert L.nfm_stoch_gram_workspace_bytes(p, q) == 0
    assert L.nfm_stoch_gram(5, 1, 1, 10, p8, p8, 64, 1 << 30, 64, 0, None) == EDTYPE
    assert L.nfm_stoch_gram(0, 1, 1, -1, p8, p8, 64, 1 << 30, 64, 0, None) == EINVAL
    assert L.nfm_stoch_gram(0, 1, 1, 10, p8, p8, 64, 1 << 30, None, 0, None) == EINVAL
    for p, q in [(1, 1), (2, 1), (1, 5), (4, 4), (3, 5), (8, 8)]:
        need = L.nfm_stoch_gram_workspace_bytes(p, q)
        assert need >= 2048 * 8 * (p * q if min(p, q) > 1 else max(p, q))
        assert L.nfm_stoch_gram(0, p, q, 10, p8, p8, 64, need - 1, 64, 0, None) == EWORKSPACE
    odd = (ctypes.c_void_p * 8)(*([66] * 8))
    assert L.nfm_stoch_gram(0, 2, 1, 10, odd, p8, 64, 1 << 30, 64, 0, None) == EALIGN
    assert L.nfm_stoch_gram(1, 1, 1, 10, p8, p8, 64, 1 << 30, 68, 0, None) == EALIGN      # out is double
    assert L.nfm_stoch_gram(0, 3, 5, 0, p8, p8, 64, 1 << 30, 64, 1, None) == 0           # nothing to add
    # combine: p in 0..8, q in 1..8, the scale op and its operands
    assert L.nfm_stoch_combine(0, 9, 1, 10, p8, 64, p8, p8, 0, None, None, None) == ESIZE
    assert L.nfm_stoch_combine(0, -1, 1, 10, p8, 64, p8, p8, 0, None, None, None) == ESIZE
    assert L.nfm_stoch_combine(0, 1, 0, 10, p8, 64, p8, p8, 0, None, None, None) == ESIZE
    assert L.nfm_stoch_combine(0, 1, 9, 10, p8, 64, p8, p8, 0, None, None, None) == ESIZE
    assert L.nfm_stoch_combine(3, 1, 1, 10, p8, 64, p8, p8, 0, None, None, None) == EDTYPE
    assert L.nfm_stoch_combine(0, 1, 1, -1, p8, 64, p8, p8, 0, None, None, None) == EINVAL
    assert L.nfm_stoch_combine(0, 1, 1, 10, p8, 64, p8, p8, 3, None, None, None) == EINVAL
    assert L.nfm_stoch_combine(0, 1, 1, 10, p8, None, p8, p8, 0, None, None, None) == EINVAL   # p > 0 needs C
    assert L.nfm_stoch_combine(0, 0, 1, 10, None, None, p8, p8, 1, None, None, None) == EINVAL  # RSQRT needs s
    assert L.nfm_stoch_combine(0, 0, 1, 10, None, None, p8, p8, 2, None, 64, None) == EINVAL    # ..OR_DROP needs s_ref
    assert L.nfm_stoch_combine(0, 0, 1, 10, None, None, p8, odd, 0, None, None, None) == EALIGN
    assert L.nfm_stoch_combine(1, 8, 8, 0, p8, 64, p8, p8, 0, None, None, None) == 0


def test_facade_refuses_cpu_tensors():
    import nitorch_fastmath_amd as N
    S = N.stochastic
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.trapprox(torch.eye(4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.maxeig_power(torch.eye(4).to_sparse())
    for fn in (S.trapprox, S.maxeig_power, S.vbald):
        # the reference's default for a callable is the CPU: say what to pass instead
        with pytest.raises(RuntimeError, match=r"no CPU fallback.*device='cuda'"):
            fn(lambda x: x, [4])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(lambda x: x, [4], device='cpu')
    with pytest.raises(ValueError, match='2-d'):
        S.trapprox(torch.zeros(3, 4, 4))                 # the reference's batched form (quirk Q51)
    with pytest.raises(TypeError):
        S.trapprox(lambda x: x, [4], device='cuda', dtype=torch.float16)
    with pytest.raises(ValueError, match='shape'):
        S.trapprox(lambda x: x, device='cuda')


def test_signatures_match_the_reference():
    import nitorch_fastmath_amd as N
    S = N.stochastic
    assert S.__all__ == ['trapprox', 'vbald', 'maxeig_power']                                # stochastic.py:1

    def names(fn):
        return list(inspect.signature(fn).parameters)

    def kinds(fn):
        return {k: p.kind for k, p in inspect.signature(fn).parameters.items()}
    KW, VK = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD
    assert names(S.trapprox) == ['matvec', 'shape', 'moments', 'samples', 'method', 'hutchpp',
                                 'generator', 'backend']                                      # stochastic.py:9-17
    assert names(S.vbald) == ['matvec', 'shape', 'upper', 'moments', 'samples', 'mc_samples', 'method',
                              'generator', 'backend']                                         # stochastic.py:149-158
    assert names(S.maxeig_power) == ['matvec', 'shape', 'max_iter', 'tol', 'check_every', 'generator',
                                     'backend']                                               # stochastic.py:316-322
    for fn in (S.trapprox, S.vbald, S.maxeig_power):
        k = kinds(fn)
        assert k['generator'] is KW and k['backend'] is VK
        assert all(v is inspect.Parameter.POSITIONAL_OR_KEYWORD for n, v in k.items()
                   if n not in ('generator', 'check_every', 'backend'))
    assert kinds(S.maxeig_power)['check_every'] is KW
    d = {k: p.default for k, p in inspect.signature(S.trapprox).parameters.items()}
    assert (d['shape'], d['moments'], d['samples'], d['method'], d['hutchpp']) == (None, None, 10, 'rademacher', False)
    d = {k: p.default for k, p in inspect.signature(S.vbald).parameters.items()}
    assert (d['upper'], d['moments'], d['samples'], d['mc_samples'], d['method']) == (None, 5, 5, 64, 'rademacher')
    d = {k: p.default for k, p in inspect.signature(S.maxeig_power).parameters.items()}
    assert (d['max_iter'], d['tol'], d['check_every']) == (512, 1e-6, 8)


def test_compat_package_serves_stochastic():
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        sys.modules.pop('nitorch_fastmath', None)
        nf = importlib.import_module('nitorch_fastmath')
        from nitorch_fastmath.stochastic import trapprox, vbald, maxeig_power
        import nitorch_fastmath_amd as N
        assert trapprox is N.stochastic.trapprox and vbald is N.stochastic.vbald
        assert nf.trapprox is trapprox and nf.vbald is vbald and nf.maxeig_power is maxeig_power
        assert nf.stochastic is N.stochastic and N.stochastic.trapprox is N.stochastic.__dict__['trapprox']
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))
        for k in [k for k in sys.modules if k == 'nitorch_fastmath' or k.startswith('nitorch_fastmath.')]:
            sys.modules.pop(k)


def test_vbald_fit_on_exact_moments_is_finite():
    from nitorch_fastmath_amd.stochastic import _vbald_fit
    lam = np.linspace(0.2, 1.0, 4096)
    mom = torch.tensor([np.mean(lam ** j) for j in range(1, 6)], dtype=torch.float64)
    torch.manual_seed(3)
    vals = np.array([float(_vbald_fit(mom, 64)) for _ in range(8)])
    assert np.isfinite(vals).all()
    # E[log lam] of a density on (0, 1): negative; the true value here is -0.56, and the reference's own
    # estimates on these moments scatter by tens of percent (tests/golden/stochastic_vbald.json)
    assert (vals < 0).all() and (vals > -5).all(), vals


def test_golden_vbald_is_data_only():
    g = json.load(open(os.path.join(GOLDEN, 'stochastic_vbald.json')))
    assert set(g['spectra']) == {'linear', 'sqrt'}
    for s in g['spectra'].values():
        assert len(s['reference_rel_err']) == 20 and np.isfinite(s['reference_rel_err']).all()
