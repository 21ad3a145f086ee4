#!/usr/bin/env python
"""Accuracy of the logm kernels -> profiles/logm_accuracy.md (the source of C_LOGM in tests/test_gpu_logm.py).

Per dtype and order: the worst ratio err / (D eps kappa_1(A)), err = max|K - T| / max|T| per matrix, on
  * the fixture tests/golden/logm.npz (truth: mpmath at 40 digits), and
  * N random A = expm(randn * 0.5) (truth: the float64 kernel for float32 input; for float64 input the torch
    route in float64, itself checked against mpmath on a sample of 1000 -- computed once with `--make-sample`,
    which needs no GPU, and read back from the file).

    python scripts/logm_accuracy.py --make-sample sample.npz        # CPU: inputs + 40-digit truth
    python scripts/logm_accuracy.py --sample sample.npz --out profiles/logm_accuracy.md
    python scripts/logm_accuracy.py --hard new.md      # the section on tests/golden/logm_hard.npz alone
"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ORDERS = range(1, 9)
DT = {'f32': torch.float32, 'f64': torch.float64}


def ratio(k, t, a):
    """err / (D eps kappa_1) per matrix; k in the dtype under test, t and a float64"""
    D = a.shape[-1]
    err = (k.double() - t).abs().amax((-2, -1)) / t.abs().amax((-2, -1)).clamp_min(1e-300)
    kap = torch.linalg.cond(a, 1)
    return err / (D * torch.finfo(k.dtype).eps * kap)


def cond_normalised(LM, k, t, a):
    """worst ||K - T||_F / ||T||_F / (eps cond_log(A)) over a sample, cond_log = ||L_log(A)||_2 ||A||_F / ||log A||_F
    the logarithm's own relative condition number; L_log as a D^2 x D^2 matrix from the float64 torch route's jvp"""
    from torch.func import jvp
    D = a.shape[-1]
    a = a.cuda()
    cols = []
    for q in range(D * D):
        e = torch.zeros(D * D, dtype=torch.float64, device='cuda')
        e[q] = 1
        cols.append(jvp(LM._logm_torch, (a,), (e.reshape(D, D).expand_as(a).contiguous(),))[1].reshape(-1, D * D))
    K = torch.stack(cols, -1)
    fro = lambda m: m.flatten(-2).norm(dim=-1)      # noqa: E731
    cond = torch.linalg.matrix_norm(K, 2).cpu() * fro(a).cpu() / fro(t).clamp_min(1e-300)
    err = fro(k.double().cpu() - t) / fro(t).clamp_min(1e-300)
    return float((err / (torch.finfo(k.dtype).eps * cond)).max())


def make_sample(path, n):
    import mpmath
    mpmath.mp.dps = 40
    gen = torch.Generator().manual_seed(11)
    out = {}
    for D in ORDERS:
        a = torch.linalg.matrix_exp(torch.randn(n, D, D, dtype=torch.float64, generator=gen) * 0.5)
        t = np.empty((n, D, D))
        for q in range(n):
            L = mpmath.logm(mpmath.matrix(a[q].tolist()))
            t[q] = [[float(mpmath.re(L[i, j])) for j in range(D)] for i in range(D)]
        out[f'a_{D}'], out[f't_{D}'] = a.numpy(), t
        print(D, flush=True)
    np.savez_compressed(path, **out)


HARD_HEAD = '## Hard inputs'


def hard_section():
    """The kernels (the torch route at the orders without one) on tests/golden/logm_hard.npz, in the units of
    tests/_logm_ref.py: worst per (dtype, order, class)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _logm_ref as R
    from nitorch_fastmath_amd import logm as LM
    g = R.load()
    cols = ['scale/A', 'graded/A', 'rot/A', 'unip/A', 'tri/A', 'rot/B', 'nonnormal/B']
    lines = [HARD_HEAD, '',
             'The kernels on tests/golden/logm_hard.npz (validated 60-digit truths; classes and tiers in',
             'tests/_logm_ref.py), worst per class.  m = max(1, cond_log).  Tier A (`/A`): ||K - T||_F / ||T||_F over',
             'eps m, held to C_LOGM = 128.  Tier B (`/B`): the same over eps m^2, with the number of all-NaN records',
             '(Q22) after the colon; a class moved to tier B by the generator shows in its own column with that unit.',
             '`frechet`: tier A, ||L - L_true||_F over D eps m^2 ||K||_2 ||E||_F.  `logm_solve`: ||K - T||_F / ||T||_F',
             'over D eps kappa_1(M) max(1, cond_log(M^-1 A)).  Orders 9 and 12 (and float64 8) are the torch route.',
             '', '| dtype | D | ' + ' | '.join(cols) + ' | frechet | logm_solve |',
             '|---|---|' + '---|' * (len(cols) + 2)]
    for dt, dtype in DT.items():
        for D in list(R.ORDERS[dt]) + list(R.ROUTE_ORDERS[dt]):
            rec = R.records(g, dt, D)
            k = LM.logm(torch.from_numpy(rec['x']).cuda()).cpu().numpy()
            _, r, what = R.check_logm(k, rec, dt)
            tb = rec['tier'] == R.TIER_B
            r = np.where(tb, r / R.m_of(rec['cl']), r)
            w = R.worst_by_class(r, rec)
            cells = []
            for c in cols:
                name, tier = c.split('/')
                sel = (rec['cls'] == name)
                if tier == 'B':
                    sel = sel & tb
                if not sel.any():
                    cells.append('')
                    continue
                moved = tier == 'A' and (rec['tier'][sel] == R.TIER_B).all()
                key = f'{name}/B' if moved else c
                cell = f'{w.get(key, float("nan")):.3g}'
                if moved or tier == 'B':
                    nn = sum(1 for i in np.flatnonzero(sel & tb) if what[i] == 'B:nan')
                    cell += f' (eps m^2):{nn}' if moved else f':{nn}'
                cells.append(cell)
            rf = rs = float('nan')
            if D in R.FRECHET_ORDERS:
                l = LM._frechet(torch.from_numpy(rec['x']).cuda(), torch.from_numpy(rec['E']).cuda()).cpu().numpy()
                rf = float(R.frechet_ratio(l, rec, dt)[~tb].max())
            if D in R.ORDERS[dt]:
                sm, sa, st, kap, cl = (g[f'{q}_{dt}_{D}'] for q in ('sm', 'sa', 'strue', 'skap', 'scl'))
                ks = LM._logm(torch.from_numpy(sa).cuda(), torch.from_numpy(sm).cuda()).double().cpu().numpy()
                rs = float((R.fro(ks - st) / R.fro(st) / (D * R.EPS[dt] * kap * R.m_of(cl))).max())
            lines.append(f'| {dt} | {D} | ' + ' | '.join(cells) + f' | {rf:.3g} | {rs:.3g} |')
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hard', metavar='PATH',
                    help='only the hard-input section: --out with that section replaced, written to PATH')
    ap.add_argument('--make-sample')
    ap.add_argument('--sample')
    ap.add_argument('--n', type=int, default=10 ** 6)
    ap.add_argument('--sample-n', type=int, default=1000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'logm_accuracy.md'))
    args = ap.parse_args()
    if args.make_sample:
        return make_sample(args.make_sample, args.sample_n)
    if args.hard:
        with open(args.out) as f:
            old = f.read().split('\n' + HARD_HEAD)[0].rstrip('\n')
        os.makedirs(os.path.dirname(os.path.abspath(args.hard)), exist_ok=True)
        with open(args.hard, 'w') as f:
            f.write(old + '\n\n' + '\n'.join(hard_section()) + '\n')
        return
    from nitorch_fastmath_amd import logm as LM
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'logm.npz'))
    smp = np.load(args.sample) if args.sample else None
    lines = ['# logm accuracy', '',
             'Worst err / (D eps kappa_1(A)) per matrix, err = max|K - T| / max|T| (scripts/logm_accuracy.py).',
             f'Random inputs: {args.n} matrices A = expm(randn * 0.5) per order.  `route64 vs mpmath`: the float64',
             'torch route, the truth of the float64 random column, against 40-digit mpmath on a sample of 1000.',
             '`by cond_log`: the sample again, ||K - T||_F / ||T||_F over eps cond_log(A) with the logarithm\'s own',
             'condition number cond_log = ||L_log(A)||_2 ||A||_F / ||log A||_F in place of D kappa_1(A).',
             f'`logm_solve`: {args.n // 10} pairs A = expm(randn * 0.3), M = expm(randn * 0.2), one M per A, err of',
             'logm(M^-1 A) over D eps kappa_1(M^-1 A); truth: the float64 kernel (float32), the float64 route on',
             '`torch.linalg.solve` (float64).', '',
             '| dtype | D | fixture | random | kernel vs mpmath (sample) | route64 vs mpmath (sample) | by cond_log '
             '| logm_solve |',
             '|---|---|---|---|---|---|---|---|']
    worst = 0.0
    for dt, dtype in DT.items():
        for D in ORDERS:
            x, true = torch.from_numpy(g[f'x_{dt}_{D}']), torch.from_numpy(g[f'true_{dt}_{D}'])
            k = LM.logm(x.cuda()).cpu()
            rf = float(ratio(k, true, x.double()).max())
            gen = torch.Generator(device='cuda').manual_seed(100 + D)
            a = torch.linalg.matrix_exp(torch.randn(args.n, D, D, dtype=torch.float64, device='cuda', generator=gen)
                                        * 0.5).to(dtype)
            k = LM.logm(a)
            if dtype == torch.float32:
                t = LM.logm(a.double())
            elif D == 1:                        # the kernel is log(): the route's square roots would be the error
                t = torch.log(a.cpu()).cuda()
            else:
                t = torch.cat([LM._logm_torch(c) for c in a.split(250000)])
            rr = float(ratio(k, t, a.double()).max())
            del a, k, t
            # logm(M^-1 A)
            rv = float('nan')
            if 2 <= D <= LM.FORWARD_MAX[dtype]:     # (D = 1: log(a / m) with a / m near 1 has no bounded relative error)
                ns = args.n // 10
                a = torch.linalg.matrix_exp(torch.randn(ns, D, D, dtype=torch.float64, device='cuda', generator=gen)
                                            * 0.3).to(dtype)
                m = torch.linalg.matrix_exp(torch.randn(ns, D, D, dtype=torch.float64, device='cuda', generator=gen)
                                            * 0.2).to(dtype)
                q = torch.linalg.solve(m.double(), a.double())
                t = LM._logm(a.double(), m.double()) if dtype == torch.float32 and D <= 7 else LM._logm_torch(q)
                r = ratio(LM._logm(a, m), t, q)
                rv = float(r[~torch.isnan(r)].max())
                del a, m, q, t
            rs = rt = rc = float('nan')
            if smp is not None:
                sa, st = torch.from_numpy(smp[f'a_{D}']).to(dtype), torch.from_numpy(smp[f't_{D}'])
                if dtype == torch.float32:      # the truth of the rounded input: first order is enough at eps32
                    st = LM._logm_torch(sa.double().cuda()).cpu()
                ks = LM.logm(sa.cuda()).cpu()
                rs = float(ratio(ks, st, sa.double()).max())
                rc = cond_normalised(LM, ks, st, sa.double())
                if dtype == torch.float64:
                    rt = float(ratio(LM._logm_torch(sa.cuda()).cpu(), st, sa).max())
            worst = max(worst, rf, rr, rs if rs == rs else 0.0, rv if rv == rv else 0.0)
            lines.append(f'| {dt} | {D} | {rf:.3g} | {rr:.3g} | {rs:.3g} | {rt:.3g} | {rc:.3g} | {rv:.3g} |')
            print(lines[-1], flush=True)
    c = 1
    while c < 4 * worst:
        c *= 2
    lines += ['', f'Worst measured ratio of the kernel: {worst:.3g}.  C_LOGM = the next power of two at or above',
              f'4 x that = {c}.']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(lines[-2], lines[-1])


if __name__ == '__main__':
    main()
