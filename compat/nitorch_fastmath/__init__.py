"""Import-compatible facade: put `compat/` on sys.path and `import nitorch_fastmath` resolves
the hot-path modules (`sym`, `batched`, `qr`, `reduce`, `lie` -- expm and expm_derivatives --, `logm` -- logm and meanm, which
the upstream package keeps in `lie` --, `simplex`, `special`, `sugar`, `realtransforms` and the helpers of `utils`) to the MI355X backend
`nitorch_fastmath_amd`.  Only the modules on the accelerated path exist here; the rest of
the upstream package (stochastic) is out of
scope of this backend.  `sugar` and `realtransforms` are star-imported like upstream's `__init__` does (`round` and
`trace` of `sugar` become package attributes, as they are upstream)."""
from nitorch_fastmath_amd import sym, batched, qr, reduce, lie, logm, simplex, special, sugar, realtransforms, utils  # noqa: F401
from nitorch_fastmath_amd.sym import *       # noqa: F401,F403
from nitorch_fastmath_amd.batched import *   # noqa: F401,F403
from nitorch_fastmath_amd.qr import *        # noqa: F401,F403
from nitorch_fastmath_amd.reduce import *    # noqa: F401,F403
from nitorch_fastmath_amd.sugar import *     # noqa: F401,F403
from nitorch_fastmath_amd.realtransforms import *   # noqa: F401,F403
import sys as _sys
for _m in ('sym', 'batched', 'qr', 'reduce', 'lie', 'logm', 'simplex', 'special', 'sugar', 'realtransforms', 'utils'):
    _sys.modules[__name__ + '.' + _m] = globals()[_m]
