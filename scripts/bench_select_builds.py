#!/usr/bin/env python
"""Two builds of libnfm_hip.so against each other on the long-row median / quantile rows of bench_median.py and
bench_quantile.py (rows longer than 1024: the kernels built from nfm_reduce_select.hpp).

Both libraries are loaded into ONE process and their C entry points run on the same input, workspace and output
buffers, so what differs between two timings is the library: parent, branch, parent again, each through
scripts/_timing.py.  A row is `within` when branch / faster parent <= slower parent / faster parent.  The results of
the two builds are compared bit for bit.

usage: bench_select_builds.py PARENT/libnfm_hip.so BRANCH/libnfm_hip.so > table.md"""
import ctypes
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nitorch_fastmath_amd import _lib  # noqa: E402
from nitorch_fastmath_amd._dispatch import stream_ptr  # noqa: E402
from _timing import BUILDS_HEADER, builds_row as row, load_build  # noqa: E402

dev = torch.device('cuda:0')
Q8 = [0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999]          # bench_quantile.py
MEDIAN = {torch.float32: ((1, 1 << 30), (64, 1 << 24), (1 << 14, 1 << 16)),
          torch.float64: ((1, 1 << 29), (1 << 13, 1 << 16))}   # bench_median.py, rows longer than 1024
QUANTILE = ((1, 1 << 28), (64, 1 << 24), (1 << 14, 1 << 16))   # bench_quantile.py, rows longer than 1024


ENTRIES = ('nfm_reduce_median', 'nfm_reduce_quantile', 'nfm_reduce_median_workspace_bytes',
           'nfm_reduce_quantile_workspace_bytes')


def median_call(L, x, ws, val, st):
    rows, red = x.shape
    args = (_lib.F32 if x.dtype == torch.float32 else _lib.F64, 0, rows, red, x.data_ptr(), ws.data_ptr(), ws.numel(),
            val.data_ptr(), None, st)

    def fn():
        _lib.check(L.nfm_reduce_median(*args))
    return fn


def quantile_call(L, x, interp, qs, ws, val, st):
    rows, red = x.shape
    qa = (ctypes.c_double * len(qs))(*qs)
    args = (_lib.F32 if x.dtype == torch.float32 else _lib.F64, 0, _lib.QUANTILE_INTERP[interp], rows, red, len(qs), qa,
            x.data_ptr(), ws.data_ptr(), ws.numel(), val.data_ptr(), None, st)

    def fn():
        _lib.check(L.nfm_reduce_quantile(*args))
    return fn


def main():
    P, B = load_build(sys.argv[1], ENTRIES), load_build(sys.argv[2], ENTRIES)
    st = stream_ptr(dev)
    print(BUILDS_HEADER)
    for dtype in (torch.float32, torch.float64):
        dn = str(dtype)[6:]
        for rows, red in MEDIAN[dtype]:
            x = torch.randn(rows, red, device=dev, dtype=dtype)
            ws = torch.empty(P.nfm_reduce_median_workspace_bytes(rows, red), dtype=torch.uint8, device=dev)
            val = torch.empty(rows, dtype=dtype, device=dev)
            row(f'median {dn} {rows} x {red}', median_call(P, x, ws, val, st), median_call(B, x, ws, val, st), val)
            del x, ws, val
        for rows, red in QUANTILE:
            x = torch.randn(rows, red, device=dev, dtype=dtype)
            for interp, qs, what in (('lower', [0.5], 'lower 1 q'), ('linear', [0.5], 'linear 1 q'), ('linear', Q8, 'linear 8 q')):
                ws = torch.empty(P.nfm_reduce_quantile_workspace_bytes(rows, red, len(qs)), dtype=torch.uint8, device=dev)
                val = torch.empty((len(qs), rows), dtype=dtype, device=dev)
                row(f'quantile {what} {dn} {rows} x {red}', quantile_call(P, x, interp, qs, ws, val, st),
                    quantile_call(B, x, interp, qs, ws, val, st), val)
                del ws, val
            del x


if __name__ == '__main__':
    main()
