#!/usr/bin/env python
"""Host-side cost per call of `sugar`'s solve families at 64 contiguous records (launch-bound: the facade is
the cost).  One process measures one tree, so two trees are compared by alternating processes:

    bench_sugar_latency.py [ROOT]       ROOT: the checkout whose package is measured (default: this one)

prints one markdown table; `torch.add` is the untouched row that shows the noise between runs."""
import os
import sys
import time
import torch
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nitorch_fastmath_amd import sugar as S  # noqa: E402

dev = torch.device('cuda:0')
g = torch.Generator(device=dev).manual_seed(0)


def per_call(fn, reps=2000, chunks=5):
    """median over `chunks` of the mean enqueue time of `reps` calls, us"""
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(chunks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        means.append((time.perf_counter() - t0) / reps * 1e6)
        torch.cuda.synchronize()
    return sorted(means)[chunks // 2]


n = 64
a3 = torch.randn(n, 3, 3, device=dev, generator=g) + 4 * torch.eye(3, device=dev)
b3 = torch.randn(n, 3, 3, device=dev, generator=g)
a12, b12 = torch.randn(n, 12, 3, device=dev, generator=g), torch.randn(n, 12, 3, device=dev, generator=g)
g4 = torch.randn(n, 4, 4, device=dev, generator=g)
spd4 = g4 @ g4.mT + 4 * torch.eye(4, device=dev)
rows = [
    ('torch.add (reference point)', lambda: torch.add(b3, b3)),
    ('lmdiv lu 3x3 f32', lambda: S.lmdiv(a3, b3)),
    ('lmdiv svd 3x3 f32', lambda: S.lmdiv(a3, b3, 'svd')),
    ('lmdiv 12x3 f32 (lstsq)', lambda: S.lmdiv(a12, b12)),
    ("inv(method='chol') 4x4 f32", lambda: S.inv(spd4, 'chol')),
]
print(f'| call (batch {n}) | host us/call (enqueue) |')
print('|---|---|')
for name, fn in rows:
    print(f'| {name} | {per_call(fn):.2f} |', flush=True)
