#!/usr/bin/env python
"""quantile (multi-rank radix selection, nfm_reduce_quantile) against its ruler -- reduce.median on the same tensor
in the same process -- and against the stock routes: torch.quantile where it runs, torch.sort + gather where it refuses.
usage: bench_quantile.py [--no-torch] > profiles/quantile_table.md"""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nitorch_fastmath_amd as N  # noqa: E402
from _timing import timeit  # noqa: E402

dev = torch.device('cuda:0')
with_torch = '--no-torch' not in sys.argv
R = N.reduce
Q8 = [0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999]
SHAPES = ((1, 1 << 28), (64, 1 << 24), (1 << 14, 1 << 16), (1 << 20, 1024), (1 << 22, 256), (1 << 24, 27))


def once(fn):
    """one timed run after one warm-up: the stock routes take up to seconds per call"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def sort_gather(x, q):
    """what a user of stock PyTorch writes where torch.quantile refuses the input: sort every row, gather two ranks"""
    s = torch.sort(x, dim=1).values
    p = q * (x.shape[1] - 1)
    lo = int(p)
    hi = min(lo + 1, x.shape[1] - 1)
    return torch.lerp(s[:, lo], s[:, hi], p - lo)


def stock(x, q):
    try:
        return f'{once(lambda: torch.quantile(x, q, dim=1)) * 1e3:.3f}', 'torch.quantile'
    except RuntimeError:
        pass
    try:
        return f'{once(lambda: sort_gather(x, q)) * 1e3:.3f}', 'sort + gather'
    except RuntimeError as e:           # out of memory
        return 'failed', type(e).__name__


print('# quantile: multi-rank radix selection (nfm_reduce_quantile) on MI355X, contiguous (rows, red)\n')
print('Ruler: reduce.median on the same tensor in the same process, timed three times (min .. max of the three medians '
      'of 8 launches = its own spread).  q = 0.5 for one quantile; 8 q = ' + str(Q8) + '.\n')
print('| dtype | rows x red | median ms (min .. max) | lower, 1 q ms | / median | linear, 1 q ms | / lower | linear, 8 q ms '
      '| / (8 x linear 1 q) | GB/s of one pass (lower, 1 q) | stock ms | stock route |')
print('|---|---|---|---|---|---|---|---|---|---|---|---|')
for dtype in (torch.float32, torch.float64):
    for rows, red in SHAPES:
        x = torch.randn(rows, red, device=dev, dtype=dtype)
        med = sorted(timeit(lambda: R.median(x, dim=1)) for _ in range(3))
        lower = timeit(lambda: R.quantile(x, 0.5, dim=1, interpolation='lower'))
        lin1 = timeit(lambda: R.quantile(x, 0.5, dim=1))
        lin8 = timeit(lambda: R.quantile(x, Q8, dim=1))
        st = stock(x, 0.5) if with_torch else ('not run', '')
        gbs = rows * red * x.element_size() / lower / 1e9
        print(f'| {str(dtype)[6:]} | {rows} x {red} | {med[1] * 1e3:.3f} ({med[0] * 1e3:.3f} .. {med[2] * 1e3:.3f}) | '
              f'{lower * 1e3:.3f} | {lower / med[1]:.2f} | {lin1 * 1e3:.3f} | {lin1 / lower:.2f} | {lin8 * 1e3:.3f} | '
              f'{lin8 / (8 * lin1):.2f} | {gbs:.0f} | {st[0]} | {st[1]} |', flush=True)
        del x
print('\nGB/s = rows x red x element size / time of the whole call: rows longer than 1024 make one streaming pass per '
      '11-bit digit of the key (3 for float32, 6 for float64) and, for linear, one successor pass more (expected '
      '4/3 and 7/6 of lower); rows up to 1024 are read once, whatever the number of q.  The median of rows of up to '
      '2 x 128 (float64: 2 x 64) elements runs its one-row-per-lane sorting networks, which quantile does not have '
      '(DESIGN 7).')

if with_torch:
    print('\n## inputs of about 16 M elements\n')
    print('| dtype | rows x red | ours linear, 1 q ms | ours linear, 8 q ms | torch.quantile 1 q ms | torch.quantile 8 q ms |')
    print('|---|---|---|---|---|---|')
    for dtype in (torch.float32, torch.float64):
        for rows, red in ((15, 1 << 20), (1 << 14, 1000), (1 << 19, 27)):
            x = torch.randn(rows, red, device=dev, dtype=dtype)
            q8 = torch.tensor(Q8, device=dev, dtype=dtype)
            a1 = timeit(lambda: R.quantile(x, 0.5, dim=1))
            a8 = timeit(lambda: R.quantile(x, Q8, dim=1))
            try:
                t1 = f'{once(lambda: torch.quantile(x, 0.5, dim=1)) * 1e3:.3f}'
                t8 = f'{once(lambda: torch.quantile(x, q8, dim=1)) * 1e3:.3f}'
            except RuntimeError:
                t1 = t8 = 'refused'
            print(f'| {str(dtype)[6:]} | {rows} x {red} | {a1 * 1e3:.3f} | {a8 * 1e3:.3f} | {t1} | {t8} |', flush=True)
            del x
