#!/usr/bin/env python
"""Two builds of the Cholesky kernels of sym (nfm_symchol.hip) against each other, through the C entry points
nfm_sym_chol and nfm_sym_chol_backward -> profiles/symchol_tile_ab.md.

Written for the record-movement experiment of nfm_symchol.hip: PARENT built with -DNFM_SYMCHOL_TILE=0 (every Op under the
spectral kernels' rule: from N = 5, float64 N = 4, a lane fetches and stores its own record), BRANCH with
-DNFM_SYMCHOL_TILE=1 (every Op through the LDS tile at every order).  The 33 objects of nfm_symchol.hip link into a
library of their own, which is all the two entries need:

    make -C nitorch_fastmath_amd/csrc -j8 symchol-exp SYMCHOL_DEFS=-DNFM_SYMCHOL_TILE=0 SYMCHOL_EXP=build/exp/tile0
    make -C nitorch_fastmath_amd/csrc -j8 symchol-exp SYMCHOL_DEFS=-DNFM_SYMCHOL_TILE=1 SYMCHOL_EXP=build/exp/tile1

Both libraries are loaded into ONE process and run on the same input and output buffers: parent, branch, parent again
(scripts/_timing.py: builds_row).  Rows: both dtypes, N in {4, 5, 6, 8}, contiguous records (2^22 at N = 4, 2^20 above);
the factor, 'Linv', logdet, logpdf and the gradient of logpdf.

usage: bench_symchol_builds.py build/exp/tile0/libnfm_symchol.so build/exp/tile1/libnfm_symchol.so > table.md
exit status 1 when a row's bits differ."""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import BUILDS_HEADER, builds_row, load_build  # noqa: E402
from nitorch_fastmath_amd._dispatch import Batch, launch  # noqa: E402
from bench_symchol import records  # noqa: E402

ENTRIES = ['nfm_sym_chol', 'nfm_sym_chol_backward']
SIZES = ((4, 1 << 22), (5, 1 << 20), (6, 1 << 20), (8, 1 << 20))


def main():
    parent, branch = (load_build(p, ENTRIES) for p in sys.argv[1:3])
    print(BUILDS_HEADER, flush=True)
    same = True
    for dtype in (torch.float32, torch.float64):
        for N, n in SIZES:
            x = records(n, N, dtype)
            K, dev = x.shape[-1], x.device
            v = torch.randn(n, N, dtype=dtype, device=dev)
            g = torch.randn(n, dtype=dtype, device=dev)
            # (row, NFM_CHOL_* op, backward, inputs, components of the result (None: a scalar))
            for name, op, bwd, ins, width in (('factor', 0, False, [x], K), ('Linv', 3, False, [x, v], N),
                                              ('logdet', 5, False, [x], None), ('logpdf', 8, False, [x, v], None),
                                              ('logpdf backward', 8, True, [x, v, g], K + N)):
                out = torch.empty((n,) if width is None else (n, width), dtype=dtype, device=dev)
                ncs = [1] * min(len(ins), 2) + ([0] if len(ins) == 3 else []) + [0 if width is None else 1]
                b = Batch((n,), ins + [out], ncs)
                slots = None if len(ins) >= 2 else (0, None, 1)

                def run(L):
                    launch(L.nfm_sym_chol_backward if bwd else L.nfm_sym_chol, dev, dtype, (N, op), b, slots=slots)

                same &= builds_row(f'{name} {str(dtype)[6:]} N={N}', lambda: run(parent), lambda: run(branch), out)[1]
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
