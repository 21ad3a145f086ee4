"""Import-compatible facade: put `compat/` on sys.path and `import nitorch_fastmath` resolves
the hot-path modules (`sym`, `batched`, `qr`, `reduce`, `lie` -- expm and expm_derivatives --, `logm` -- logm and meanm, which
the upstream package keeps in `lie` --, `simplex`, `special`, `sugar`, `realtransforms`, `stochastic` and the helpers of `utils`) to the MI355X backend
`nitorch_fastmath_amd`: every module that upstream's `__init__` star-imports is served.  `sugar`, `realtransforms`
and `stochastic` are star-imported like upstream's `__init__` does (`round` and `trace` of `sugar`, `trapprox`,
`vbald` and `maxeig_power` of `stochastic` become package attributes, as they are upstream)."""
from nitorch_fastmath_amd import sym, batched, qr, reduce, lie, logm, simplex, special, sugar, realtransforms, stochastic, utils  # noqa: F401
from nitorch_fastmath_amd.sym import *       # noqa: F401,F403
from nitorch_fastmath_amd.batched import *   # noqa: F401,F403
from nitorch_fastmath_amd.qr import *        # noqa: F401,F403
from nitorch_fastmath_amd.reduce import *    # noqa: F401,F403
from nitorch_fastmath_amd.sugar import *     # noqa: F401,F403
from nitorch_fastmath_amd.realtransforms import *   # noqa: F401,F403
from nitorch_fastmath_amd.stochastic import *   # noqa: F401,F403
import sys as _sys
for _m in ('sym', 'batched', 'qr', 'reduce', 'lie', 'logm', 'simplex', 'special', 'sugar', 'realtransforms', 'stochastic', 'utils'):
    _sys.modules[__name__ + '.' + _m] = globals()[_m]
