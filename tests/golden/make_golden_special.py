#!/usr/bin/env python
"""Generate tests/golden/special.npz from the REAL reference `special.py`, scipy.special and mpmath (build
container only) and write the reference part of profiles/special_accuracy.md.

    python tests/golden/make_golden_special.py <path of the reference package nitorch_fastmath>

What the file holds and how C follows from the reference's own error: tests/_special_fixture.py.
"""
import importlib.util
import os
import sys
import warnings
import numpy as np
import torch
import mpmath as mp
import scipy.special as sc

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _special_fixture as F  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NFM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_special.py <path of the reference package nitorch_fastmath> (or NFM_REFERENCE)')
mp.mp.dps = 40
NPTS, NGRAD = 192, 64


def load_ref():
    spec = importlib.util.spec_from_file_location('nfm_reference_special', os.path.join(REF, 'special.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def loguniform(gen, lo, hi, n):
    u = torch.rand(n, dtype=torch.float64, generator=gen)
    return torch.exp(np.log(lo) + u * (np.log(hi) - np.log(lo))).float().sort()[0]


def f64(v):
    return float(v) if abs(v) < mp.mpf('1e308') else float('inf') * (1 if v > 0 else -1)


def mp_besseli(nu, z, mode):
    i = mp.besseli(nu, mp.mpf(float(z)))
    return f64(i) if mode == 0 else f64(i * mp.exp(-mp.mpf(float(z)))) if mode == 1 else f64(mp.log(i))


def mp_ratio(nu, z):
    z = mp.mpf(float(z))
    return mp.besseli(nu + 1, z) / mp.besseli(nu, z)


def call(R, kind, prm, x):
    if kind in ('besseliP', 'besseliA'):
        return R.besseli(prm['nu'], x.clone(), prm['mode'])
    if kind == 'ratio':
        return R.besseli_ratio(prm['nu'], x.clone(), prm['N'], prm['K'])
    return R.mvdigamma(x.clone(), prm['order'])


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20261017)
    out = {}
    edge = np.float32(15.0 / 4.0)
    near = [edge]
    for k in range(3):
        near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(10))]
    zP = torch.cat([loguniform(gen, 1e-6, 80.0, NPTS), torch.tensor(np.array(near, dtype=np.float32))]).sort()[0]
    zA = loguniform(gen, 1e-6, 500.0, 256)
    out['zP'], out['zA'] = zP.numpy(), zA.numpy()
    for order in F.ORDERS:
        out[f'x_{order}'] = (loguniform(gen, 1e-3, 1e4, NPTS) + (order - 1) / 2).numpy()
    gi = {k: np.linspace(0, len(out[k]) - 1, NGRAD).astype(np.int64) for k in list(out)}
    for k, v in gi.items():
        out['gidx_' + k] = v
    worst = {('P', 'f32'): {}, ('A', 'f32'): {}, ('A', 'f64'): {}}
    fx = F.Fixture.__new__(F.Fixture)
    fx.z = out
    todo = []
    for kind, key, prm in F.cases():
        ik = F.input_key(kind, prm)
        x32 = torch.from_numpy(out[ik])
        x64 = x32.double()
        r32 = call(R, kind, prm, x32).numpy()
        r64 = call(R, kind, prm, x64).numpy()
        out['R32_' + key] = r32
        if kind == 'besseliA':
            nu, m = prm['nu'], prm['mode']
            T = np.array([mp_besseli(nu, z, m) for z in out[ik]])
            chk = sc.ive(nu, x64.numpy())           # scipy agrees with mpmath (on the log: no overflow)
            lg = np.log(chk) + x64.numpy()
            tl = T if m == 2 else np.array([mp_besseli(nu, z, 2) for z in out[ik]])
            ok = np.isfinite(lg) & (chk > 1e-300)
            assert np.abs(lg[ok] - tl[ok]).max() <= 1e-13 * (1 + np.abs(tl[ok])).max(), (nu, m)
            out['R64_' + key] = r64
        else:
            T = r64
        out['T_' + key] = T
        if kind == 'mvdigamma':
            xs = [x64.numpy() + (1 - p) / 2 for p in range(1, prm['order'] + 1)]
            out['B_' + key] = np.array([sum(1 + abs(mp.psi(0, mp.mpf(float(v[i])))) for v in xs) for i in range(len(xs[0]))],
                                       dtype=np.float64)
        todo.append((kind, key, prm, r32, r64))
        # gradients on NGRAD points
        idx = gi[ik]
        G, GB = np.zeros(NGRAD), np.zeros(NGRAD)
        for j, i in enumerate(idx):
            z = mp.mpf(float(out[ik][i]))
            if kind == 'mvdigamma':
                t = [mp.psi(1, z + mp.mpf(1 - p) / 2) for p in range(1, prm['order'] + 1)]
                g, gb = sum(t), sum(1 + abs(v) for v in t)
            elif kind == 'ratio':
                r = mp.mpf(float(T[i]))
                a, b = r * r, (2 * prm['nu'] + 1) * r / z
                g, gb = 1 - a - b, 1 + a + b
            else:
                nu, m = prm['nu'], prm['mode']
                r, a = mp_ratio(nu, z), mp.mpf(nu) / z
                t = mp.mpf(float(T[i]))
                if m == 2:
                    g, gb = r + a, 1 + r + a
                else:
                    g = t * (r + a - (1 if m == 1 else 0))
                    gb = abs(t) * (r + a + (1 if m == 1 else 0))
                    if kind == 'besseliA':
                        gb *= 1 + abs(mp.log(mp.besseli(nu, z))) + z
            G[j], GB[j] = f64(g), f64(gb)
        out['G_' + key], out['GB_' + key] = G, GB
    # the reference's own worst ratio to the C = 1 bounds
    for kind, key, prm, r32, r64 in todo:
        T = out['T_' + key]
        if kind == 'besseliA':
            ok = F.valid(prm['nu'], out['zA'].astype(np.float64))
            for dt, r in (('f32', r32), ('f64', r64)):
                # the reference forms exp(f) before the factors below 1: it overflows up to three decades early
                use = ok & ~(np.isinf(r) & (np.abs(T) > float(np.finfo(F.NP[dt]).max) / 1024))
                worst[('A', dt)][key] = F.ratio(r[use], T[use], fx.bound(kind, key, prm, dt)[use], dt)
        else:
            worst[('P', 'f32')][key] = F.ratio(r32, T, fx.bound(kind, key, prm, 'f32'), 'f32')
    for (g, dt), w in worst.items():
        rr = max(w.values())
        out[f'ref_ratio_{g}_{dt}'] = np.float64(rr)
        out[f'C_{g}_{dt}'] = np.float64(2.0 ** int(np.ceil(np.log2(4 * rr))))
    out['ref_ratio_P_f64'], out['C_P_f64'] = out['ref_ratio_P_f32'], out['C_P_f32']   # see _special_fixture.py
    # special values: the documented pattern; finite entries from mpmath / the reference in float64
    sp = np.array(F.SPECIAL, dtype=np.float64)
    out['special_x'] = sp
    for nu in F.NU_P + F.NU_A:
        for m in range(3):
            e = np.empty(len(sp))
            for i, z in enumerate(sp):
                if np.isnan(z):
                    e[i] = np.nan
                elif np.isinf(z):
                    e[i] = (np.inf, 0.0, np.inf)[m]
                elif z == 0:
                    e[i] = ((1.0, 1.0, 0.0) if nu == 0 else (0.0, 0.0, -np.inf))[m]
                elif nu in F.NU_P:
                    e[i] = float(call(R, 'besseliP', dict(nu=nu, mode=m), torch.tensor([z], dtype=torch.float64))[0])
                else:
                    e[i] = mp_besseli(nu, z, m)
            out[f'special_bi_{F.tag(nu)}_{m}'] = e
    for nu in F.NU_R:
        for N, K in F.NK:
            e = call(R, 'ratio', dict(nu=nu, N=N, K=K), torch.from_numpy(sp)).numpy()
            e[sp == 0], e[np.isinf(sp)] = 0.0, 1.0
            out[f'special_br_{F.tag(nu)}_{N}_{K}'] = e
    spd = np.array(F.SPECIAL_DG, dtype=np.float64)
    out['special_dg_x'] = spd
    for order in F.ORDERS:
        out[f'special_dg_{order}'] = call(R, 'mvdigamma', dict(order=order), torch.from_numpy(spd)).numpy()
        # the derivative at the same points: the trigamma sum from mpmath where every term is finite
        e = np.full(len(spd), np.nan)
        for i, v in enumerate(spd):
            xs = [mp.mpf(float(v) + (1 - p) / 2) for p in range(1, order + 1)]    # the shifts round in float64, as upstream
            if np.isfinite(v) and not any(x <= 0 and x == mp.floor(x) for x in xs):
                e[i] = f64(sum(mp.psi(1, x) for x in xs))
        out[f'special_dg_grad_{order}'] = e
    np.savez_compressed(F.PATH, **out)
    print(F.PATH, os.path.getsize(F.PATH), 'bytes')
    for k in sorted(out):
        if k.startswith(('ref_ratio', 'C_')):
            print(k, float(out[k]))
    prof = os.path.join(os.path.dirname(os.path.dirname(HERE)), 'profiles', 'special_accuracy.md')
    kernel = ''
    if os.path.exists(prof):
        txt = open(prof).read()
        if '## Kernels' in txt:
            kernel = txt[txt.index('## Kernels'):]
    with open(prof, 'w') as f:
        f.write('# special: accuracy against the truth\n\n'
                'Worst ratio |result - truth| / bound (C = 1; bounds and truths in tests/_special_fixture.py) over the cases\n'
                'of tests/golden/special.npz.\n\n## Reference (CPU)\n\n| group, dtype | worst case | worst ratio | C |\n|---|---|---|---|\n')
        for (g, dt), w in worst.items():
            k = max(w, key=w.get)
            f.write(f'| {g}, {dt} | {k} | {w[k]:.3g} | {float(out[f"C_{g}_{dt}"]):g} |\n')
        f.write('\nGroup A is measured on the range where the reference is right (z > 2 nu and z >= 2 thr).  Outside it the\n'
                'reference misses the same bounds by orders of magnitude (tests/test_special_host.py asserts that).\n\n')
        f.write('## Allowances of the tests beyond the bounds above\n\n'
                'Both come from the number formats (tests/_special_fixture.py), not from any result.\n\n'
                '| allowance | float32 | float64 |\n|---|---|---|\n')
        cnt = {dt: [0, 0, 0, 0] for dt in ('f32', 'f64')}
        for dt in cnt:
            step = float(np.finfo(F.NP[dt]).smallest_subnormal)
            for kind, key, prm in F.cases():
                gi, use = fx.grad_points(kind, key, prm, dt)
                T = np.abs(out['T_' + key])
                b = fx.bound(kind, key, prm, dt) * float(out[f'C_{F.group(kind)}_{dt}'])
                cnt[dt][0] += int(((b < step) & (T > 0) & np.isfinite(T)).sum())
                cnt[dt][1] += T.size
                cnt[dt][2] += int((~use).sum())
                cnt[dt][3] += len(gi)
        f.write('| one subnormal step added to every bound: forward elements whose C x bound is below that step | '
                + ' | '.join(f'{cnt[dt][0]} of {cnt[dt][1]}' for dt in cnt) + ' |\n')
        f.write("| gradient points of besseli None / 'norm' left out because the saved output is subnormal | "
                + ' | '.join(f'{cnt[dt][2]} of {cnt[dt][3]}' for dt in cnt) + ' |\n\n')
        f.write(kernel or '## Kernels\n\n(not measured yet)\n')


if __name__ == '__main__':
    main()
