#!/usr/bin/env python
"""Throughput of logm.logm / logm(M^-1 A) (nfm_logm.hip) and of logm.meanm -> profiles/logm_table.md.

Inputs: A = expm(randn * 0.3).  Per row: matrices/s, the mean number of square roots s, of Denman-Beavers
steps and the mean series degree the kernel runs (replayed on the host in float64 with the kernel's rules,
nfm_logm_ops.hpp, on a sample), the share of the larger roofline bound (FLOPs over the vector peak -- FP32
157.3 TF, FP64 78.6 TF -- or algorithmic bytes over 8 TB/s; FLOPs counted as for expm, 2 D^3 per product, plus
2 D^3 per inverse), and the ratio to the torch route (`_logm_torch`, the only device baseline: torch has no
matrix_log) on a batch of `--n-torch` matrices.  For scale only, the reference's path restated (`.cpu()`,
scipy.linalg.logm per matrix, back) at 10^4 matrices.

    python scripts/bench_logm.py [--md out.md] [--n 10000000]"""
import argparse
import os
import sys
import time
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
from nitorch_fastmath_amd import logm as LM  # noqa: E402

PEAK = {torch.float32: 157.3e12, torch.float64: 78.6e12}
BW = 8.0e12


def replay(a, dtype):
    """host replay (float64 arithmetic, the dtype's constants) of the square roots, steps and degree"""
    a = a.double().cpu()
    D = a.shape[-1]
    eps = torch.finfo(dtype).eps
    eye = torch.eye(D, dtype=torch.float64)
    roots = steps = deg = 0
    for y in a:
        while float((y - eye).abs().sum(0).max()) > LM.THETA:
            m = y.clone()
            while True:
                e_prev = float((m - eye).abs().sum(0).max())
                mi = torch.linalg.inv(m)
                y = 0.5 * (y + y @ mi)
                m = 0.5 * (eye + 0.5 * (m + mi))
                steps += 1
                if float((m - eye).abs().sum(0).max()) <= 4 * D * eps or e_prev <= eps ** 0.5:
                    break
            roots += 1
        z = (y - eye) @ torch.linalg.inv(y + eye)
        zn = float(z.abs().sum(0).max())
        k, pw = 0, zn
        while k < 16 and pw > eps * 0.125 * (2 * k + 1):
            pw *= zn * zn
            k += 1
        deg += k
    n = len(a)
    return roots / n, steps / n, deg / n


def spread(n, D, dtype, scale=0.3):
    return torch.linalg.matrix_exp(torch.randn(n, D, D, dtype=torch.float64, device='cuda') * scale).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--n', type=int, default=10 ** 7)
    ap.add_argument('--n-torch', type=int, default=10 ** 5)
    args = ap.parse_args()
    out = ['# logm / meanm on MI355X (scripts/bench_logm.py)', '',
           f'Matrices A = expm(randn * 0.3), n per row ({args.n:.0e}, half of it at D = 8); steady-state medians.',
           f'`x torch route`: per-matrix time of the torch route on a batch of {args.n_torch:.0e} (it does not fit n)',
           'over the kernel\'s per-matrix time on its n.', '',
           '| op | dtype | D | n | 1e9 matrices/s | roots s | steps | degree | roofline share | x torch route |',
           '|---|---|---|---|---|---|---|---|---|---|']
    for dtype in (torch.float32, torch.float64):
        for D in (2, 3, 4, 6, 8):
            if D > LM.FORWARD_MAX[dtype]:
                continue
            n = args.n if D < 8 else args.n // 2
            a = spread(n, D, dtype)
            s, st, dg = replay(a[:200], dtype)
            flops = 2 * D ** 3 * (st * 2 + 3 + dg + 1)          # per step: inverse + product; tail: inverse, 3 products, Horner
            byts = 2 * D * D * a.element_size()
            small = a[:args.n_torch]
            tt = timeit(lambda: LM._logm_torch(small), reps=3) / len(small)
            m1 = spread(1, D, dtype, 0.1)
            for name, fn in (('logm', lambda: LM._logm(a)), ('logm_solve (M stride 0)', lambda: LM._logm(a, m1))):
                t = timeit(fn) / n
                fl = flops + (2 * D ** 3 if 'solve' in name else 0)
                sc, sb = fl / t / PEAK[dtype], byts / t / BW
                out.append(f'| {name} | {str(dtype)[6:]} | {D} | {n:.0e} | {1e-9 / t:.3f} | {s:.2f} | {st:.2f} | {dg:.2f} | '
                           f'{max(sc, sb):.3f} ({"compute" if sc >= sb else "memory"}) | {tt / t:.0f} |')
                print(out[-1], flush=True)
            del a
    # the reference's path restated, for scale
    try:
        import scipy.linalg
        a = spread(10 ** 4, 4, torch.float64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.stack([torch.as_tensor(scipy.linalg.logm(m.cpu().numpy())) for m in a]).cuda()
        torch.cuda.synchronize()
        out += ['', f'Reference path restated (`.cpu()`, scipy.linalg.logm per matrix, back), 10^4 float64 4x4: '
                    f'{(time.perf_counter() - t0) / 1e4 * 1e6:.1f} us per matrix.']
    except ImportError:
        pass
    # meanm: 16 rigid 4x4 matrices, and 1e5 such sets at once
    B = torch.zeros(6, 4, 4, dtype=torch.float64, device='cuda')
    for k in range(3):
        B[k, k, 3] = 1
    for k, (i, j) in enumerate([(0, 1), (0, 2), (1, 2)]):
        B[3 + k, i, j], B[3 + k, j, i] = 1, -1
    for nsets in (1, 10 ** 5):
        p = torch.randn(nsets, 16, 6, dtype=torch.float64, device='cuda') * 0.3
        mats = torch.linalg.matrix_exp(torch.einsum('snf,fij->snij', p, B))
        mats = mats[0] if nsets == 1 else mats
        iters = LM._meanm(mats, 1024, 1e-20)[1]
        t = timeit(lambda: LM.meanm(mats), reps=3)
        out += ['', f'meanm, {nsets} set(s) of 16 rigid 4x4 (float64): {iters} iterations, {t / iters * 1e6:.1f} us per '
                    f'iteration, {t * 1e3:.3f} ms in all.']
        print(out[-1], flush=True)
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
