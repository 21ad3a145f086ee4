"""nitorch_fastmath_amd -- MI355X-native (gfx950) backend for the per-element
small-matrix hot path of nitorch-fastmath: `sym`, `batched`, `qr`, the NaN-omitting
reductions of `reduce`, the matrix exponential of `lie`, the matrix logarithm / exponential barycentre
of `logm`, the implicit-class softmax family of `simplex`, the Bessel / digamma functions of `special` and the small solves of `sugar`
(lmdiv / rmdiv / solvevec / inv), the cosine / sine transforms of `realtransforms`, and the probes, inner products and
orthogonalisation around the caller's operator in `stochastic` (trapprox / vbald / maxeig_power),
behind the reference's own Python function signatures.

Host code is Python on PyTorch-ROCm (device memory, streams); the arithmetic is
hand-written HIP in `libnfm_hip.so`, reached through the C ABI of include/nfm_hip.h.
There is no CPU path: importing works anywhere, calling needs the built library and
GPU tensors.
"""
from . import sym, batched, reduce, qr, lie, logm, simplex, special, sugar, realtransforms, stochastic, utils  # noqa: F401
from .sym import *       # noqa: F401,F403
from .batched import *   # noqa: F401,F403
from .qr import *        # noqa: F401,F403
# `reduce` shadows builtins (min, max, sum) exactly like the reference's star-import does
# (`__init__.py:1-10`); keep them namespaced at package level as well.
from ._lib import LIB_PATH, lib as _load_lib  # noqa: F401


def is_built():
    """True when the HIP shared library has been compiled in-tree."""
    import os
    return os.path.exists(LIB_PATH)
