#!/usr/bin/env python
"""Registers and throughput of the two-matrix spectral kernels of sym (nfm_sympencil.hip) -> profiles/sympencil_table.md.

    python scripts/bench_sympencil.py --resources [--times FILE] [--md out.md]     (no GPU: reads the built objects)
    python scripts/bench_sympencil.py [--md out.md] [--n 4194304]                  (on the GPU)

Each mode rewrites its own section of the file and leaves the other one alone.

Resources: VGPRs (AGPRs), LDS and waves per SIMD of every instantiation, from the code objects
(scripts/kernel_resources.py); --times FILE adds the compile time of each part ("part seconds" per line).

Speed: N in {2, 3, 6, 7, 8} (7: the float64 caps), both dtypes, 2^22 pairs of compact SPD records, contiguous.  Per row: records/s, the share of
the HBM roofline (8 TB/s) on the algorithmic bytes (3 K elements per record forward: two reads and a write,
K = N (N + 1) / 2; 4 K for the gradient of a function; 2 K + 1 for the distance, 4 K + 1 for its gradients) and the
ratios to
  * the composition route of the facade (nitorch_fastmath_amd/_sympencil.py: sym_sqrtm, sym_rsqrtm, torch products,
    sym_funm, torch products and pack; backward: autograd through it);
  * for the functions, forward: the chain of the module's own kernels a user would write,
    sym_rsqrtm -> sym_to_full -> sym_matmul -> sym_funm -> (sym_sqrtm -> sym_to_full ->) sym_matmul.
A ratio above 1 means the fused kernel is faster."""
import argparse
import glob
import os
import re
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BW = 8.0e12
HEAD = {'resources': '## Resources (scripts/bench_sympencil.py --resources)', 'speed': '## Speed (scripts/bench_sympencil.py)'}
TITLE = '# sym_pencil_funm, sym_geneigvals, sym_dist: registers and speed on MI355X'


def write_section(path, which, lines):
    """replace the section `which` of the file (created with the title if missing)"""
    parts = {'resources': [], 'speed': []}
    if path and os.path.exists(path):
        cur = None
        for line in open(path).read().splitlines():
            hit = [k for k, h in HEAD.items() if line == h]
            if hit:
                cur = hit[0]
            elif cur:
                parts[cur].append(line)
    parts[which] = lines
    text = TITLE + '\n\n' + '\n\n'.join(HEAD[k] + '\n' + '\n'.join(parts[k]).strip('\n') for k in ('resources', 'speed')
                                       if parts[k]) + '\n'
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text)
    print(text)


def resources(args):
    import kernel_resources as KR
    rows = KR.collect(sorted(glob.glob(os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc', 'nfm_sympencil_*.o'))))
    kinds = {0: 'run-time modes', 1: 'contiguous', 2: 'channel-first', 3: 'channel-first, 512 lanes'}
    from nitorch_fastmath_amd import _lib
    caps = ', '.join(f'{name} {_lib.lib().nfm_sym_pencil_max_order(0, op)} / {_lib.lib().nfm_sym_pencil_max_order(1, op)}'
                     for op, name in enumerate(('function', 'its gradient', 'eigenvalues and distance',
                                                'gradients of the distance')))
    out = ['', 'One row per instantiation of rec_kernel.  No kernel has a private segment.  The caps '
           f'(`nfm_sym_pencil_max_order`, float32 / float64): {caps}.', '',
           '| Op | dtype | N | kernel form | registers (VGPRs + AGPRs) | of them AGPRs | LDS bytes (static) | scratch | waves / SIMD |',
           '|---|---|---|---|---|---|---|---|---|']
    tab = []
    for k in rows:
        m = re.search(r'rec_kernel<(float|double), (?:nfm::)?(Pencil\w+)<\w+, (\d+)(?:, (true|false))?>, (\d)>', k['kernel'])
        if not m:
            continue
        op = m.group(2) + ({'true': ' (distance)', 'false': ' (eigenvalues)'}.get(m.group(4), ''))
        tab.append((op, m.group(1), int(m.group(3)), int(m.group(5)), k))
    for op, t, n, kind, k in sorted(tab, key=lambda r: r[:4]):
        # the register count is the whole allocation of the unified file (AGPRs included), in granules of 8
        waves = min(8, 512 // (((int(k['vgpr']) + 7) // 8) * 8))
        out.append(f"| {op} | {t} | {n} | {kinds[kind]} | {k['vgpr']} | {k['agpr']} | {k['lds_static']} | "
                   f"{k['scratch']} | {waves} |")
    if args.times:
        t = dict(line.split() for line in open(args.times) if line.strip())
        out += ['', 'Compile time per object in seconds, 16 at a time (part = 1 + dtype * 16 + op * 4 + pair of orders; '
                'op: function, its gradient, eigenvalues / distance, gradients of the distance): '
                + ', '.join(f'{p}: {float(t[str(p)]):.0f}' for p in range(33) if str(p) in t) + '.']
    write_section(args.md, 'resources', out)


def spd(n, N, dtype):
    g = torch.randn(n, N, N, dtype=dtype, device='cuda')
    a = g @ g.transpose(-1, -2) / N + torch.eye(N, dtype=dtype, device='cuda')
    r = list(range(N)) + [i for i in range(N) for j in range(i + 1, N)]
    c = list(range(N)) + [j for i in range(N) for j in range(i + 1, N)]
    return a[:, r, c].contiguous()


def speed(args):
    from _timing import timeit
    from nitorch_fastmath_amd import _lib, _sympencil as C, sym as S
    n = args.n
    out = ['', f'{n} pairs of compact SPD records per row, contiguous, steady-state medians.  `x composition`: the time '
           'of the composition of single-matrix calls (_sympencil.py; backward: autograd through it) over the time of '
           'the kernel; `x kernel chain`: the same for sym_rsqrtm -> sym_to_full -> sym_matmul -> sym_funm -> sym_sqrtm '
           '-> sym_to_full -> sym_matmul (functions, forward).', '',
           '| function | dtype | N | direction | 1e9 records/s | HBM roofline share | x composition | x kernel chain |',
           '|---|---|---|---|---|---|---|---|']
    slower = []
    for dtype in (torch.float32, torch.float64):
        for N in (2, 3, 6, 7, 8):
            a, b = spd(n, N, dtype), spd(n, N, dtype)
            g = torch.randn_like(a)
            g1 = torch.randn(n, dtype=dtype, device='cuda')
            K, es = a.shape[-1], a.element_size()
            cases = []
            for fn, p in (('pow', 0.3), ('sqrt', None), ('rsqrt', None), ('log', None), ('exp', None)):
                code = _lib.FUN[fn]
                pp = 0.0 if p is None else p
                def chain(fn=fn, p=p):
                    c = S.sym_matmul(S.sym_to_full(S.sym_rsqrtm(a)), b)
                    return S.sym_matmul(S.sym_to_full(S.sym_sqrtm(a)), S.sym_funm(c, fn, p=p))
                cases.append((f'sym_pencil_funm {fn}', 'forward', _lib.PENCIL_OP_FUNM, 3 * K,
                              lambda fn=fn, p=p: S.sym_pencil_funm(a, b, fn, p=p),
                              lambda code=code, p=p: C.pencil_funm(a, b, code, p), chain))
                if fn != 'sqrt':          # (sqrt is pow 1/2: the same kernel path as pow)
                    def comp_bwd(code=code, p=p):
                        br = b.clone().requires_grad_(True)
                        y = C.pencil_funm(a, br, code, p)
                        return lambda: torch.autograd.grad(y, br, g, retain_graph=True)
                    cases.append((f'sym_pencil_funm {fn}', 'gradient (mat)', _lib.PENCIL_OP_FUNM_BACKWARD, 4 * K,
                                  lambda code=code, pp=pp: S._pencil_backward(a, b, g, code, pp, None), comp_bwd, None))
                if fn == 'pow':          # the base gradient of the powers: the backward kernel on swapped operands
                    def comp_base(code=code, p=p):
                        ar = a.clone().requires_grad_(True)
                        y = C.pencil_funm(ar, b, code, p)
                        return lambda: torch.autograd.grad(y, ar, g, retain_graph=True)
                    cases.append((f'sym_pencil_funm {fn}', 'gradient (base, swapped kernel)', _lib.PENCIL_OP_FUNM_BACKWARD,
                                  4 * K, lambda code=code, p=p: S._pencil_backward(b, a, g, code, 1.0 - p, None),
                                  comp_base, None))
                if fn == 'log':          # the base gradient of log / exp IS the composition (forward and backward of it)
                    cases.append((f'sym_pencil_funm {fn}', 'gradient (base, composition)', _lib.PENCIL_OP_FUNM, 4 * K,
                                  lambda code=code: S._pencil_grad_composed(a, b, g, code, None, 0), None, None))
            cases.append(('sym_geneigvals', 'forward', _lib.PENCIL_OP_EIG, 2 * K + N,
                          lambda: S.sym_geneigvals(b, a), lambda: C.geneigvals(a, b), None))
            cases.append(('sym_dist squared', 'forward', _lib.PENCIL_OP_EIG, 2 * K + 1,
                          lambda: S.sym_dist(a, b, squared=True), lambda: C.dist(a, b, True), None))

            def dist_bwd():
                ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
                d = C.dist(ar, br, True)
                return lambda: torch.autograd.grad(d, (ar, br), g1, retain_graph=True)
            cases.append(('sym_dist squared', 'gradients (both)', _lib.PENCIL_OP_DIST_BACKWARD, 4 * K + 1,
                          lambda: S._pencil_dist_backward(a, b, g1, _lib.PENCIL_DIST2, None), dist_bwd, None))
            for name, direction, op, elems, kern, comp, chain in cases:
                tag = f'| {name} | {str(dtype)[6:]} | {N} | {direction} |'
                if N > S._pencil_cap(dtype, op):
                    out.append(f'{tag} composition route (above the cap) | - | - | - |')
                    continue
                if comp is None:          # no fused kernel to compare with: the route's own time
                    t = timeit(kern, reps=5)
                    out.append(f'{tag} {n / t * 1e-9:.3f} | {elems * es * n / t / BW:.3f} | - | - |')
                    print(out[-1], flush=True)
                    continue
                t = timeit(kern)
                if 'gradient' in direction:
                    comp = comp()          # builds the graph once, times the backward alone
                tc = timeit(comp, reps=5)
                tk = timeit(chain, reps=5) if chain is not None else None
                out.append(f'{tag} {n / t * 1e-9:.3f} | {elems * es * n / t / BW:.3f} | {tc / t:.1f} | '
                           + (f'{tk / t:.1f} |' if tk else '- |'))
                print(out[-1], flush=True)
                if min(tc, tk or tc) < t:
                    slower.append(f'{name} {str(dtype)[6:]} N={N} {direction}: {min(tc, tk or tc) / t:.2f}x the composition')
                del comp
            del a, b, g, g1, cases
            torch.cuda.empty_cache()
    out += ['', 'Cases slower than the composition: ' + ('; '.join(slower) if slower else 'none') + '.']
    write_section(args.md, 'speed', out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--n', type=int, default=1 << 22)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--times', default=None)
    args = ap.parse_args()
    resources(args) if args.resources else speed(args)


if __name__ == '__main__':
    main()
