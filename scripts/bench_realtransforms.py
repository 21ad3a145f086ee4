#!/usr/bin/env python
"""Throughput of the real-transform kernels (nfm_rt.hip, nfm_rt_mm.hip) against the module's own torch.fft
composition, forced, on the same tensors.

`(2^22, N)` along the last axis and `(N, 2^22)` along the first at N in {8, 32, 64, 128, 256}, and `dctn` over all
axes of a 192^3 and a 182 x 218 x 182 volume, float32 and float64, DCT-II 'ortho'.  Per row: the route the
facade takes ('lane': one line per lane, 'mm': the matrix-core kernel), its time (median of event-timed launches
after a settle phase, scripts/_timing.py), the achieved bytes/s at 2 x elements x itemsize per pass (one read,
one write) as a share of the HBM copy ceiling measured in the same process (a device-to-device `copy_` of the
same tensor), and composition time / kernel time.  The composition is `_apply(..., force_torch=True)`: what
serves an axis when no kernel does.  Two informational columns for the 2^22-line rows: the matrix-core kernel
through its C entry wherever the facade does not route to it (N = 64, or a length above `mm_max_len`), and
`torch.matmul` against the dense matrix.

`mm_max_len(dtype)` (NFM_RT_MM_MAX_LEN_F32 / _F64 of nfm_rt.hip) is to be the largest of {128, 256} at which the
matrix-core kernel is not slower than the composition in both layouts, 64 if neither; `max_len(dtype)` the same
for the lane kernels over {64, 128, 256}.

    python scripts/bench_realtransforms.py [--md out.md] [--log2n 22]"""
import argparse
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N  # noqa: E402
from nitorch_fastmath_amd import _lib  # noqa: E402
from nitorch_fastmath_amd._dispatch import call  # noqa: E402

RT = N.realtransforms
KIND, TYPE, NORM = 0, 2, 'ortho'


def mm_entry(x, d, out):
    """nfm_rt_transform_mm along axis d of a contiguous tensor, whatever the facade's routing"""
    outer, n, inner = RT._view(x, d)
    call(_lib.lib().nfm_rt_transform_mm, x.device, RT._KERNEL_DTYPES[x.dtype], KIND, TYPE, _lib.RT_NORMS[NORM], 0,
         n, outer, inner, x.data_ptr(), out.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=22)
    a = ap.parse_args()
    lines = ['| case | dtype | N | route | kernel ms | share of copy ceiling | composition ms | composition / kernel '
             '| mm entry ms | matmul ms |',
             '|---|---|---|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(0)
    nline = 1 << a.log2n
    for dtype in (torch.float32, torch.float64):
        cases = [(f'({nline}, N) last axis', (nline, n), [1], n) for n in (8, 32, 64, 128, 256)]
        cases += [(f'(N, {nline}) first axis', (n, nline), [0], n) for n in (8, 32, 64, 128, 256)]
        cases += [('192^3 dctn, all axes', (192, 192, 192), [0, 1, 2], 192)]
        cases += [('182 x 218 x 182 dctn, all axes', (182, 218, 182), [0, 1, 2], 218)]
        for name, shape, dims, n in cases:
            x = torch.randn(shape, device='cuda', dtype=dtype, generator=gen)
            y = torch.empty_like(x)
            t_copy = timeit(lambda: y.copy_(x))
            by = 2 * x.numel() * x.element_size() * len(dims)
            ceiling = 2 * x.numel() * x.element_size() / t_copy
            routes = {RT._route(x, x.shape[d], False) for d in dims}
            route = '+'.join(sorted(routes))
            t_entry = t_mat = None
            with torch.no_grad():
                tb = timeit(lambda: RT._apply(x, dims, KIND, TYPE, NORM, False, force_torch=True))
                t = None if 'torch' in routes else timeit(lambda: RT._apply(x, dims, KIND, TYPE, NORM, False))
                if len(dims) == 1 and n >= 64:
                    if route != 'mm':
                        t_entry = timeit(lambda: mm_entry(x, dims[0], y))
                    M = RT._apply(torch.eye(n, device='cuda', dtype=dtype), [0], KIND, TYPE, NORM, False)
                    Mt = M.t().contiguous()
                    t_mat = timeit((lambda: torch.matmul(x, Mt, out=y)) if dims == [1] else
                                   (lambda: torch.matmul(M, x, out=y)))
            ms = lambda v: '' if v is None else f'{v * 1e3:.3f}'  # noqa: E731
            if t is None:
                r = f'| {name} | {str(dtype)[6:]} | {n} | torch | not served | | {tb * 1e3:.3f} | |'
            else:
                r = (f'| {name} | {str(dtype)[6:]} | {n} | {route} | {t * 1e3:.3f} | {by / t / ceiling:.2f} | '
                     f'{tb * 1e3:.3f} | {tb / t:.2f} |')
            r += f' {ms(t_entry)} | {ms(t_mat)} |'
            print(r, flush=True)
            lines.append(r)
            del x, y
            torch.cuda.empty_cache()
    if a.md:
        with open(a.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
