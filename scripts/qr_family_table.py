#!/usr/bin/env python
"""Assemble the tables of profiles/qr_family_accuracy.md from the `qr-family` lines that
tests/test_qr_family_host.py and tests/test_gpu_qr_family.py print (run them with -s and keep the output).

usage: qr_family_table.py NAME=LOG [NAME=LOG ...] > tables.md
  one column group per NAME (e.g. before=host_parent.log after=host.log gpu=gpu.log).  A row is
  (dtype, operation, family): the operation's variants (basis, side, triangle, with / without reflectors) are merged
  by their worst ratio; the columns are the orders.  Ratios are error / bound without the constant: the bar is 16."""
import collections
import sys

BAR = 16.0


def base(op):
    return op.split(' ')[0]


def parse(path):
    """{(dtype, operation, family): {order: worst ratio}}"""
    out = collections.defaultdict(dict)
    for line in open(path):
        line = line.lstrip('.FEsx')                     # (pytest's progress marks share the line with -s)
        if not line.startswith('qr-family |'):
            continue
        _, tag, dn, n, op, fam, ratio, _ = [x.strip() for x in line.split('|')]
        key, n, ratio = (dn, base(op), fam), int(n), float(ratio)
        out[key][n] = max(out[key].get(n, 0.0), ratio)
    return out


def fmt(x):
    if x is None:
        return ''
    s = 'inf' if x == float('inf') else (f'{x:.2g}' if x >= 100 else f'{x:.3g}')
    return f'**{s}**' if x > BAR else s


def main():
    cols = [a.split('=', 1) for a in sys.argv[1:]]
    data = {name: parse(path) for name, path in cols}
    keys = list(dict.fromkeys(k for d in data.values() for k in d))        # in the order the tests print them
    keys.sort(key=lambda k: (k[0], k[1]))                                   # (stable: families keep that order)
    orders = sorted({n for d in data.values() for v in d.values() for n in v})
    for dn in ('f32', 'f64'):
        for name, _ in cols:
            rows = [k for k in keys if k[0] == dn and k in data[name]]
            if not rows:
                continue
            print(f'\n### {dn}, {name}\n')
            print('| operation | family | ' + ' | '.join(f'n={n}' for n in orders) + ' |')
            print('|---|---|' + '---|' * len(orders))
            for k in rows:
                print(f'| {k[1]} | {k[2]} | ' + ' | '.join(fmt(data[name][k].get(n)) for n in orders) + ' |')
    # the summary: worst ratio per (operation, family group), over dtypes and orders
    print('\n### summary: worst ratio over dtypes and orders\n')
    print('| operation | families | ' + ' | '.join(name for name, _ in cols) + ' |')
    print('|---|---|' + '---|' * len(cols))
    groups = collections.defaultdict(lambda: collections.defaultdict(float))
    for name, _ in cols:
        for (dn, op, fam), v in data[name].items():
            g = 'tiny rows' if fam.startswith('tiny rows') else ('tiny border' if fam.startswith('tiny border') else ('tiny' if fam.startswith('tiny') else
                                                                 ('rank-deficient' if 'rank' in fam or fam == 'outer' else
                                                                  ('axis-aligned' if fam.startswith('axis') else 'other'))))
            groups[(op, g)][name] = max(groups[(op, g)][name], max(v.values()))
    for (op, g), v in sorted(groups.items()):
        print(f'| {op} | {g} | ' + ' | '.join(fmt(v.get(name)) for name, _ in cols) + ' |')


if __name__ == '__main__':
    main()
