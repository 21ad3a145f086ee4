"""profiles/qr_large_orders_parity.md from the `parity` lines that tests/test_gpu_qr_large_orders.py prints:

    python -m pytest -m gpu -s tests/test_gpu_qr_large_orders.py > log.txt
    python scripts/qr_large_parity_table.py log.txt > profiles/qr_large_orders_parity.md
"""
import sys

HEAD = """# QR family at orders 9..16: parity with the oracle, per kernel form

One row per dtype x order x operation x form, from `tests/test_gpu_qr_large_orders.py` on an MI355X
(`scripts/qr_large_parity_table.py`).  1000 + n seeded records (`tests/_qr_large_ref.py`).

- `contiguous`: back-to-back records, the register form (`qr_large_*`) where `qr_large_fits` allows, the
  LDS-resident form (`qr_lds_kernel`) elsewhere;  `matrix-first`, `two-level` and the mixed `rq_hessenberg`
  operands: always the LDS-resident form.
- `relerr`: worst batch max-norm relative error against the oracle over the operation's outputs.  `eig_sym fast`
  rows compare SORTED values (the fast sweeps promise no order), so their `= oracle` is the position-by-position
  answer and is expected to be `no`.
- `= oracle`: every output bit-identical to the oracle's;  `= contiguous`: bit-identical to the contiguous call.

| dtype | order | operation | form | relerr | = oracle | = contiguous |
|---|---|---|---|---|---|---|
"""


def main(path):
    rows = []
    for line in open(path):
        i = line.find('parity | ')      # (pytest's progress dots may precede it on the line)
        if i < 0:
            continue
        f = [x.strip() for x in line[i:].rstrip('\n').split('|')]
        if len(f) == 8:
            rows.append(f[1:])
    yn = {'True': 'yes', 'False': 'no', 'self': 'itself'}
    rows.sort(key=lambda r: (r[0], int(r[1]), r[2], r[3]))
    sys.stdout.write(HEAD)
    for dn, n, op, form, err, bo, bc in rows:
        sys.stdout.write(f'| {dn} | {n} | {op} | {form} | {err} | {yn[bo]} | {yn[bc]} |\n')


if __name__ == '__main__':
    main(sys.argv[1])
