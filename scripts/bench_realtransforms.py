#!/usr/bin/env python
"""Throughput of the real-transform kernels (nfm_rt.hip) against the module's own torch.fft composition, forced,
on the same tensors.

`(2^22, N)` along the last axis and `(N, 2^22)` along the first at N in {8, 32, 64, 128, 256}, and a 192^3
`dctn` over all axes, float32 and float64, DCT-II 'ortho'.  Per row: time (median of event-timed launches
after a settle phase, scripts/_timing.py), the achieved bytes/s at 2 x elements x itemsize per pass (one read,
one write) as a share of the HBM copy ceiling measured in the same process (a device-to-device `copy_` of the
same tensor), and composition time / kernel time.  Lengths above the cap of the loaded library
(`realtransforms.max_len`) are reported as 'not served': measuring them takes a library built with
`-DNFM_RT_MAX_LEN_F32=256 -DNFM_RT_MAX_LEN_F64=256`.  `max_len(dtype)` is to be the largest of {64, 128, 256} at
which the kernel is not slower than the composition in both layouts.

    python scripts/bench_realtransforms.py [--md out.md] [--log2n 22]"""
import argparse
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N  # noqa: E402

RT = N.realtransforms
KIND, TYPE, NORM = 0, 2, 'ortho'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=22)
    a = ap.parse_args()
    lines = ['| case | dtype | N | kernel ms | share of copy ceiling | composition ms | composition / kernel |',
             '|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(0)
    nline = 1 << a.log2n
    for dtype in (torch.float32, torch.float64):
        cases = [(f'({nline}, N) last axis', (nline, n), [1], n) for n in (8, 32, 64, 128, 256)]
        cases += [(f'(N, {nline}) first axis', (n, nline), [0], n) for n in (8, 32, 64, 128, 256)]
        cases += [('192^3 dctn, all axes', (192, 192, 192), [0, 1, 2], 192)]
        for name, shape, dims, n in cases:
            x = torch.randn(shape, device='cuda', dtype=dtype, generator=gen)
            y = torch.empty_like(x)
            t_copy = timeit(lambda: y.copy_(x))
            del y
            by = 2 * x.numel() * x.element_size() * len(dims)
            with torch.no_grad():
                tb = timeit(lambda: RT._apply(x, dims, KIND, TYPE, NORM, False, force_torch=True))
                if n <= RT.max_len(dtype):
                    t = timeit(lambda: RT._apply(x, dims, KIND, TYPE, NORM, False))
                    ceiling = 2 * x.numel() * x.element_size() / t_copy
                    r = (f'| {name} | {str(dtype)[6:]} | {n} | {t * 1e3:.3f} | {by / t / ceiling:.2f} | {tb * 1e3:.3f} | '
                         f'{tb / t:.2f} |')
                else:
                    r = f'| {name} | {str(dtype)[6:]} | {n} | not served | | {tb * 1e3:.3f} | |'
            print(r, flush=True)
            lines.append(r)
            del x
            torch.cuda.empty_cache()
    if a.md:
        with open(a.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
