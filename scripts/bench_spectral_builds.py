#!/usr/bin/env python
"""Two builds of libnfm_hip.so against each other on the spectral kernels of sym (nfm_symfun.hip, nfm_sympencil.hip),
through the C entry points: nfm_sym_funm and its backward, nfm_sym_pencil_funm and its backward, nfm_sym_pencil_eig
(eigenvalues and squared distance) and nfm_sym_pencil_dist_backward.

Both libraries are loaded into ONE process and run on the same input and output buffers: parent, branch, parent again
(scripts/_timing.py: builds_row).  Rows: both dtypes, N in {2, 3, 6, the cap of the (dtype, entry)}, contiguous records
and channel-first, 2^22 records (2^20 for float64 from N = 7 on).  Inputs: well-conditioned SPD records; 3 % of them are
multiples of the identity (and, for a pencil, a B that is a multiple of A), so the a == b branches of the divided
differences run.

usage: bench_spectral_builds.py PARENT/libnfm_hip.so BRANCH/libnfm_hip.so [--n RECORDS] [--only SUBSTRING] > table.md
exit status 1 when a row's bits differ."""
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
ENTRIES = ('nfm_sym_funm', 'nfm_sym_funm_backward', 'nfm_sym_funm_max_order', 'nfm_sym_pencil_funm',
           'nfm_sym_pencil_funm_backward', 'nfm_sym_pencil_eig', 'nfm_sym_pencil_dist_backward',
           'nfm_sym_pencil_max_order')
LOG, POW = (_lib.FUN['log'], 0.0, 0, 0.0), (_lib.FUN['pow'], 0.3, 0, 0.0)     # (fn, p, has_min, vmin)
# (row name, entry, its scalars after M, the code of its *_max_order, inputs, components of the result (K, N or 1))
ROWS = (('sym_funm log', 'nfm_sym_funm', LOG, 0, 'a', 'K'),
        ('sym_funm_backward log', 'nfm_sym_funm_backward', LOG, 1, 'ag', 'K'),
        ('sym_pencil_funm pow 0.3', 'nfm_sym_pencil_funm', POW, _lib.PENCIL_OP_FUNM, 'ab', 'K'),
        ('sym_pencil_funm_backward pow 0.3', 'nfm_sym_pencil_funm_backward', POW, _lib.PENCIL_OP_FUNM_BACKWARD, 'abg', 'K'),
        ('sym_pencil_eig eigenvalues', 'nfm_sym_pencil_eig', (_lib.PENCIL_EIG,), _lib.PENCIL_OP_EIG, 'ab', 'N'),
        ('sym_pencil_eig distance^2', 'nfm_sym_pencil_eig', (_lib.PENCIL_DIST2,), _lib.PENCIL_OP_EIG, 'ab', '1'),
        ('sym_pencil_dist_backward', 'nfm_sym_pencil_dist_backward', (_lib.PENCIL_DIST2,), _lib.PENCIL_OP_DIST_BACKWARD,
         'ab1', '2K'))


def compact(a):
    N = a.shape[-1]
    r = list(range(N)) + [i for i in range(N) for j in range(i + 1, N)]
    c = list(range(N)) + [j for i in range(N) for j in range(i + 1, N)]
    return a[:, r, c].contiguous()


def inputs(n, N, dtype):
    """compact SPD a, b (3 % of the records: a = s I, b = t a), a cotangent g and a scalar cotangent"""
    gen = torch.Generator(device=dev).manual_seed(N)
    eye = torch.eye(N, dtype=dtype, device=dev)
    out = []
    for _ in range(2):
        g = torch.randn(n, N, N, dtype=dtype, device=dev, generator=gen)
        out.append(g @ g.transpose(-1, -2) / N + eye)
        del g
    a, b = out
    rep = torch.rand(n, device=dev, generator=gen) < 0.03
    s = 1 + torch.rand(n, 1, 1, dtype=dtype, device=dev, generator=gen)
    a = torch.where(rep[:, None, None], s * eye, a)
    b = torch.where(rep[:, None, None], (2 * s - 1) * a, b)
    a, b = compact(a), compact(b)
    return {'a': a, 'b': b, 'g': torch.randn(a.shape, dtype=dtype, device=dev, generator=gen),
            '1': torch.randn(n, 1, dtype=dtype, device=dev, generator=gen)}


def entry_call(L, entry, dtype, M, scalars, tensors, st):
    """the call of one build on (n, components) tensors of any strides; the result is the last one"""
    b = Batch(tensors[0].shape[:-1], tensors, [1] * len(tensors))
    args = (dtype_code(dtype), M, *scalars, b.n_outer, b.n_inner, *[byref(o) for o in b.operands], st)
    fn = getattr(L, entry)
    return lambda: _lib.check(fn(*args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('branch')
    ap.add_argument('--n', type=int, default=1 << 22)
    ap.add_argument('--only', default='', help='rows whose name contains this')
    args = ap.parse_args()
    P, B = load_build(args.parent, ENTRIES), load_build(args.branch, ENTRIES)
    st = stream_ptr(dev)
    print(BUILDS_HEADER)
    same_all = True
    for dtype in (torch.float32, torch.float64):
        code, dn = dtype_code(dtype), str(dtype)[6:]
        caps = [(B.nfm_sym_funm_max_order if 'pencil' not in entry else B.nfm_sym_pencil_max_order)(code, op)
                for _, entry, _, op, _, _ in ROWS]
        for N in sorted({2, 3, 6, *caps}):
            n = args.n >> 2 if dtype == torch.float64 and N >= 7 else args.n
            x = inputs(n, N, dtype)
            K = x['a'].shape[-1]
            for (name, entry, scalars, _, ins, comp), cap in zip(ROWS, caps):
                if N > cap or (N > 6 and N != cap) or args.only not in name:
                    continue
                for layout in ('contiguous', 'channel-first'):
                    # channel-first: (components, n) in memory, seen as (n, components)
                    cf = (lambda t: t.t().contiguous().t()) if layout == 'channel-first' else (lambda t: t)
                    val = cf(torch.empty(n, {'K': K, 'N': N, '1': 1, '2K': 2 * K}[comp], dtype=dtype, device=dev))
                    ops = [cf(x[k]) for k in ins] + [val]
                    _, same = builds_row(f'{name} {dn} N={N} {layout} n=2^{n.bit_length() - 1}',
                                         entry_call(P, entry, dtype, N, scalars, ops, st),
                                         entry_call(B, entry, dtype, N, scalars, ops, st), val)
                    same_all &= same
                    del ops, val
            del x
            torch.cuda.empty_cache()
    return 0 if same_all else 1


if __name__ == '__main__':
    sys.exit(main())
