#!/usr/bin/env python
"""Worst observed fraction of each error bound of tests/test_gpu_stochastic.py -> profiles/stochastic_accuracy.md.

The tests print the figure behind every bound before they assert it; this script runs them once on the GPU with
output capture off and keeps the maximum per (check, dtype).

    python scripts/stochastic_accuracy.py [--md profiles/stochastic_accuracy.md]"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (row label, pattern with groups (dtype, fraction), the bound)
CHECKS = [
    ('fill, Gaussian', r'^[.FEsx]*gaussian (f\d\d) offset \d+ n \d+: worst \|err\| / bound = (\S+)', '8 eps max(1, r) against the float64 model'),
    ('gram', r'^[.FEsx]*gram (f\d\d) \(\d,\d\) n \d+: worst err / bound = (\S+)', 'n eps64 sum |x_i y_i| against extended-precision sums'),
    ('combine', r'^[.FEsx]*combine (f\d\d) \(\d,\d\) n \d+: worst err / bound = (\S+)', '(p + 2) eps (|y| + sum |x| |c|), elementwise'),
    ('orth', r'^[.FEsx]*orth (f\d\d) cond \S+ m \d: .*fraction of bound (\S+)', '2 loss(Householder) + 4 m eps on the kept columns'),
    ('trapprox, dense 256 x 256', r'^[.FEsx]*dense (f\d\d) \w+ hutchpp=\w+: .*fraction (\S+)', '2 err(reference) + 4 m N eps |t| against the float64 model'),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    args = ap.parse_args()
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_stochastic.py'), '-m', 'gpu',
                        '-q', '-s'], capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-6000:] + r.stderr[-2000:])
    worst = {}
    for line in r.stdout.splitlines():
        for label, pat, _ in CHECKS:
            m = re.match(pat, line)
            if m:
                key = (label, m.group(1))
                worst[key] = max(worst.get(key, 0.0), float(m.group(2)))
    lines = [f'Worst observed fraction of each bound of tests/test_gpu_stochastic.py (pytest: {r.stdout.strip().splitlines()[-1]}).',
             '', '| check | bound | float32 | float64 |', '|---|---|---|---|']
    for label, _, bound in CHECKS:
        lines.append(f'| {label} | {bound} | {worst.get((label, "f32"), float("nan")):.2e} | {worst.get((label, "f64"), float("nan")):.2e} |')
    print('\n'.join(lines))
    if args.md:
        open(args.md, 'w').write('\n'.join(lines) + '\n')
    return r.returncode


if __name__ == '__main__':
    sys.exit(main())
