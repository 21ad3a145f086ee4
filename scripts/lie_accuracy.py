#!/usr/bin/env python
"""Accuracy table of lie.expm / expm_derivatives against the 40-digit truth of tests/golden/lie.npz:
per (dtype, D) the worst error max|K - T| / max|T| of the kernel and of the reference, and the worst ratio
err / (D eps (1 + ||X||_1)) -- the constant C of the test bound C D eps (1 + ||X||_1).  The Frechet kernels get the
same per input class of tests/_lie_ref.py: float32 at D = 1..4 and both depths, float64 on tests/golden/lie_frechet.npz.
The forward kernels by input class (`--forward`: that section alone): the interleaved batches of
tests/test_gpu_lie_forward.py in units of D eps max(1, cond_exp(X)) on the Frobenius error; without a GPU the kernel
cells say "not measured".

    python scripts/lie_accuracy.py [--md out.md] [--forward]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nitorch_fastmath_amd as N  # noqa: E402


def forward_section():
    """worst ||K - T||_F / (||T||_F D eps max(1, cond_exp)) per (dtype, order, class): the kernel, the float model of
    its formulas (tests/_lie_ref.expm_model) and torch.linalg.matrix_exp in the same dtype on the CPU"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _lie_ref as R
    from nitorch_fastmath_amd import lie
    gpu = torch.cuda.is_available()
    out = ['', '| forward kernels | D | class | records | kernel worst C | model worst C | matrix_exp worst C | worst cond_exp |',
           '|---|---|---|---|---|---|---|---|']
    for dn in ('f32', 'f64'):
        dtype = R.DT[dn]
        for D in range(1, lie.FORWARD_MAX[dtype] + 1):
            x, idx, t, cond = R.fwd_case(D, dn)
            classes = R.fwd_classes(dn, D)
            cm = R.fwd_worst(R.fwd_c(R.expm_model(x, dtype)[0], t, x, dtype, cond), idx, classes)
            cr = R.fwd_worst(R.fwd_c(torch.linalg.matrix_exp(x) if D > 1 else torch.exp(x), t, x, dtype, cond), idx, classes)
            ck = R.fwd_worst(R.fwd_c(lie.expm(x.cuda()).cpu(), t, x, dtype, cond), idx, classes) if gpu else None
            wc = R.fwd_worst(cond, idx, classes)
            for q, cls in enumerate(classes):
                name = R.cname(cls)
                kernel = f'{ck[name]:.2f}' if gpu else 'not measured'
                out.append(f'| {dn} | {D} | {name} | {int((idx == q).sum())} | {kernel} | {cm[name]:.2f} | {cr[name]:.2f} | '
                           f'{wc[name]:.3g} |')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--forward', action='store_true', help='the forward-kernels-by-class section alone')
    args = ap.parse_args()
    if args.forward:
        out = '\n'.join(forward_section()[1:]) + '\n'
        print(out)
        if args.md:
            open(args.md, 'w').write(out)
        return
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'lie.npz'))
    lines = ['| dtype | D | kernel worst err | reference worst err | kernel worst C | reference worst C (finite) |',
             '|---|---|---|---|---|---|']
    worst = 0.0
    for dt, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        eps = torch.finfo(dtype).eps
        for D in range(1, 9):
            x, ref, true = (g[f'{k}_{dt}_{D}'] for k in ('x', 'ref', 'true'))
            k = N.lie.expm(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
            den = np.abs(true).max((1, 2))
            ek = np.abs(k - true).max((1, 2)) / den
            er = np.abs(ref.astype(np.float64) - true).max((1, 2)) / den
            b = D * eps * (1 + np.abs(x.astype(np.float64)).sum(1).max(1))
            ck, cr = ek / b, er / b
            worst = max(worst, ck.max())
            lines.append(f'| {dt} | {D} | {ek.max():.2e} | {np.nanmax(er):.2e} | {ck.max():.2f} | '
                         f'{np.nanmax(np.where(np.isfinite(cr), cr, 0)):.3g} |')
    dl = ['', '| derivatives (float64) | D | dX worst err | hX worst err | worst C |', '|---|---|---|---|---|']
    worst_d = 0.0
    for D in (2, 3, 4):
        x = torch.from_numpy(g[f'dx_{D}']).cuda()
        _, dX, hX = N.lie.expm_derivatives(x, grad_X=True, hess_X=True)
        xn = g[f'dx_{D}']
        b = D * 2.0 ** -52 * (1 + np.abs(xn).sum(1).max(1))
        e1 = np.abs(dX.cpu().numpy() - g[f'dtrue_dX_{D}']).reshape(2, -1).max(1) / np.abs(g[f'dtrue_dX_{D}']).reshape(2, -1).max(1)
        e2 = np.abs(hX.cpu().numpy() - g[f'dtrue_hX_{D}']).reshape(2, -1).max(1) / np.abs(g[f'dtrue_hX_{D}']).reshape(2, -1).max(1)
        c = max((e1 / b).max(), (e2 / b).max())
        worst_d = max(worst_d, c)
        dl.append(f'| | {D} | {e1.max():.2e} | {e2.max():.2e} | {c:.2f} |')
    # Frechet kernels by input class (tests/_lie_ref.py): 2000 records per class, float32 against the float64 block
    # identities with the float32 identities as reference; float64 on the 96-record 40-digit fixture
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _lie_ref as R
    from nitorch_fastmath_amd import lie
    fl = ['', '| Frechet kernels | D | depth | class | kernel worst err | kernel worst C | reference worst err | '
          'reference worst C |', '|---|---|---|---|---|---|---|---|']

    def rows(dn, D, depth, x, a, b, truth, ref, where):
        dtype = R.DT[dn]
        bb = b if depth == 2 else None
        k = lie._frechet(x.cuda(), a.cuda(), None if bb is None else bb.cuda(), 10000, 1e-32).cpu()
        t = truth(bb)
        r = ref(bb)
        for cls, sl in where:
            ek, er = R.err(k[sl], t[sl]), R.err(r[sl], t[sl])
            u = R.unit(x[sl], dtype)
            fl.append(f'| {dn} | {D} | {depth} | {R.cname(cls)} | {float(ek.max()):.2e} | {float((ek / u).max()):.2f} | '
                      f'{float(er.max()):.2e} | {float((er / u).max()):.2f} |')

    for D in (1, 2, 3, 4):
        x, a, b, where = R.all_inputs(2000, D, 'f32')
        for depth in (1, 2):
            rows('f32', D, depth, x, a, b, lambda bb: R.frechet_truth64(x, a, bb),
                 lambda bb: R.frechet_ref(x, a, bb, torch.float32), where)
    for D in R.FIXTURE_ORDERS:
        x, a, b, L, L2 = R.fixture_records(D)
        for depth in (1, 2):
            rows('f64', D, depth, x, a, b, lambda bb: L if bb is None else L2,
                 lambda bb: R.frechet_truth64(x, a, bb), R.fixture_classes())
    # 10^6 random matrices (randn * 0.7) against matrix_exp in float64 on the device, as tests/test_gpu_lie.py::test_scale
    sl = ['', '| 10^6 x randn * 0.7 vs matrix_exp (float64) | D | worst err | worst C |', '|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(7)
    for dtype in (torch.float32, torch.float64):
        for D in (3, 4):
            x = (torch.randn(10 ** 6, D, D, dtype=torch.float64, device='cuda', generator=gen) * 0.7).to(dtype)
            t = torch.linalg.matrix_exp(x.double())
            err = (N.lie.expm(x).double() - t).abs().amax((-2, -1)) / t.abs().amax((-2, -1))
            c = err / (D * torch.finfo(dtype).eps * (1 + x.double().abs().sum(-2).amax(-1)))
            sl.append(f'| {str(dtype)[6:]} | {D} | {float(err.max()):.2e} | {float(c.max()):.2f} |')
    out = '\n'.join(lines + dl + fl + forward_section() + sl + ['', f'worst C on the fixture: expm {worst:.2f}, derivatives {worst_d:.2f}']) + '\n'
    print(out)
    if args.md:
        open(args.md, 'w').write(out)


if __name__ == '__main__':
    main()
