#!/usr/bin/env python
"""Two builds of libnfm_hip.so against each other on the QR entry points the range guard of the building blocks
touches -- nfm_qr_hessenberg (general and symmetric) and nfm_qr_qr_hessenberg -- and on nfm_qr_eig_sym, which it must
not move: 2e6 contiguous N(0, 1) records, 3x3 float32 and 6x6 float64.

Both libraries are loaded into ONE process and run on the same input and output buffers: parent, branch, parent again
(scripts/_timing.py: builds_row).  A branch time beyond the spread of the parent's own two runs is a slowdown.

usage: bench_qr_family_builds.py PARENT/libnfm_hip.so BRANCH/libnfm_hip.so [--n RECORDS] > table.md
exit status 1 when a row's bits differ (N(0, 1) records are inside the guard's window: the bits must not change)."""
import argparse
import os
import sys
from ctypes import byref
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nitorch_fastmath_amd import _lib  # noqa: E402
from nitorch_fastmath_amd._dispatch import Batch, dtype_code, stream_ptr  # noqa: E402
from _timing import BUILDS_HEADER, builds_row, load_build  # noqa: E402

dev = torch.device('cuda:0')
ENTRIES = ('nfm_qr_hessenberg', 'nfm_qr_qr_hessenberg', 'nfm_qr_eig_sym')
# (row name, entry, its scalars after the dtype as a function of N, input, length of the packed output record)
ROWS = (('hessenberg', 'nfm_qr_hessenberg', lambda N: (N, 0, 1, 0), 'a', lambda N: N * N),
        ('hessenberg reflectors', 'nfm_qr_hessenberg', lambda N: (N, 0, 1, 1), 'a', lambda N: N * N + (N - 2) * (N - 1)),
        ('hessenberg_sym', 'nfm_qr_hessenberg', lambda N: (N, 1, 1, 0), 'a', lambda N: N * N),
        ('qr_hessenberg', 'nfm_qr_qr_hessenberg', lambda N: (N,), 'hz', lambda N: 2 * N * N),
        ('eig_sym', 'nfm_qr_eig_sym', lambda N: (N, 1, 0, 1024, 1e-32), 'sym', lambda N: N),
        ('eig_sym vectors', 'nfm_qr_eig_sym', lambda N: (N, 1, _lib.EIG_VECTORS, 1024, 1e-32), 'sym', lambda N: N + N * N))


def entry_call(L, entry, dtype, scalars, x, out, st):
    b = Batch(x.shape[:-2], [x], [2])
    args = (dtype_code(dtype), *scalars, b.n_outer, b.n_inner, *[byref(o) for o in b.operands], out.data_ptr(), st)
    fn = getattr(L, entry)
    return lambda: _lib.check(fn(*args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('branch')
    ap.add_argument('--n', type=int, default=2000000)
    args = ap.parse_args()
    P, B = load_build(args.parent, ENTRIES), load_build(args.branch, ENTRIES)
    st = stream_ptr(dev)
    print(BUILDS_HEADER)
    same_all = True
    for dtype, N in ((torch.float32, 3), (torch.float64, 6)):
        gen = torch.Generator(device=dev).manual_seed(N)
        a = torch.randn(args.n, N, N, dtype=dtype, device=dev, generator=gen)
        x = {'a': a, 'hz': torch.triu(a, -1), 'sym': (a + a.mT) / 2}
        for name, entry, scalars, key, rec in ROWS:
            out = torch.empty(args.n, rec(N), dtype=dtype, device=dev)
            _, same = builds_row(f'{name} {str(dtype)[6:]} {N}x{N} n={args.n}',
                                 entry_call(P, entry, dtype, scalars(N), x[key], out, st),
                                 entry_call(B, entry, dtype, scalars(N), x[key], out, st), out)
            same_all &= same
            del out
    return 0 if same_all else 1


if __name__ == '__main__':
    sys.exit(main())
