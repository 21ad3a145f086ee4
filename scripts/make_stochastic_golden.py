"""Record the spread of the REFERENCE's vbald on two spectra -> tests/golden/stochastic_vbald.json (data only).

    python scripts/make_stochastic_golden.py --reference /path/to/nitorch-fastmath

The reference's `stochastic.py` is loaded under a stub package (its `__init__` would import jitfields) and run on
the CPU in float32, its default.  Its estimate is noisy by construction -- 64 Monte-Carlo nodes, redrawn at every
loss evaluation -- so what a test of this backend's `vbald` can be held to is this recorded spread: for each
spectrum, 20 seeded runs with `upper = max(lambda)`, and the relative error of each against sum(log(lambda))."""
import argparse
import importlib
import json
import os
import sys
import types
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, RUNS = 4096, 20


def spectra(n=N):
    i = np.arange(n, dtype=np.float64)
    return {'linear': np.linspace(0.2, 1.0, n), 'sqrt': 0.1 + 0.9 * np.sqrt((i + 0.5) / n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference (holds nitorch_fastmath/stochastic.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'stochastic_vbald.json'))
    args = ap.parse_args()
    pkg = types.ModuleType('nitorch_fastmath')
    pkg.__path__ = [os.path.join(args.reference, 'nitorch_fastmath')]
    sys.modules['nitorch_fastmath'] = pkg
    S = importlib.import_module('nitorch_fastmath.stochastic')
    out = {'n': N, 'runs': RUNS, 'dtype': 'float32', 'upper': 'max', 'seed': 'torch.manual_seed(1000 + run)', 'spectra': {}}
    for name, lam64 in spectra().items():
        lam = torch.as_tensor(lam64, dtype=torch.float32)
        truth = float(np.log(lam64).sum())
        errs = []
        for run in range(RUNS):
            torch.manual_seed(1000 + run)
            ld = float(S.vbald(lambda x: x * lam, [N], upper=float(lam.max())))
            errs.append((ld - truth) / abs(truth))
        a = np.abs(errs)
        out['spectra'][name] = {'truth_logdet': truth, 'reference_rel_err': errs,
                                'abs_median': float(np.median(a)), 'abs_p75': float(np.percentile(a, 75))}
        print(name, 'truth %.2f' % truth, '|rel err| median %.3f p75 %.3f max %.3f' % (np.median(a), np.percentile(a, 75), a.max()))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
