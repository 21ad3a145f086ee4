#!/usr/bin/env python
"""Are the gfx950 kernels of two builds the same?  For a change that touches host code only.

Compares, object by object, the code objects of two build directories (or two libnfm_hip.so): the set of
kernel symbols, each kernel's metadata (VGPR, AGPR, SGPR, static LDS, scratch, max workgroup size), its
kernel descriptor and its machine code.  A whole code object is not reproducible across output paths, so
sections and symbols are compared, never file hashes: first `.text` and `.rodata` as a whole, and when
those differ (instantiations in another order) kernel by kernel, by symbol address and size.

usage: compare_kernels.py PARENT BRANCH      (two csrc directories with their *.o, or two shared libraries)
prints one line per object that differs and `N kernels, D differing`; exit status 1 when D > 0."""
import glob
import os
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_objects, kernels_of

META = ('vgpr', 'agpr', 'sgpr', 'lds_static', 'scratch', 'max_flat_workgroup_size')


def _readelf(co, what):
    return subprocess.run([f'{LLVM}/llvm-readelf', what, '--wide', co], capture_output=True, text=True).stdout


def sections(co):
    """name -> (address, file offset, size, index)"""
    out = {}
    for m in re.finditer(r'^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', _readelf(co, '--sections'), re.M):
        out[m.group(2)] = (int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16), int(m.group(1)))
    return out


def symbols(co):
    """name -> (address, size, section index) of the defined functions and objects"""
    out = {}
    for m in re.finditer(r'^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)', _readelf(co, '--symbols'), re.M):
        out[m.group(5)] = (int(m.group(1), 16), int(m.group(2)), int(m.group(4)))
    return out


class CodeObject:
    def __init__(self, path):
        self.data = open(path, 'rb').read()
        self.sec = sections(path)
        self.by_index = {v[3]: v for v in self.sec.values()}
        self.sym = symbols(path)
        self.meta = {k['symbol']: tuple(k[f] for f in META) for k in kernels_of(path)}

    def section(self, name):
        if name not in self.sec:
            return b''
        _, off, size, _ = self.sec[name]
        return self.data[off:off + size]

    def symbol(self, name):
        if name not in self.sym:
            return None
        addr, size, idx = self.sym[name]
        saddr, off, _, _ = self.by_index[idx]
        return self.data[off + addr - saddr:off + addr - saddr + size]


def descriptor(co, kernel):
    """the 64-byte kernel descriptor without its bytes 16..23, the offset from the descriptor to the kernel's
    code (it moves with the kernel's place in .text; the code itself is compared on its own)"""
    kd = co.symbol(kernel + '.kd')
    return None if kd is None else kd[:16] + kd[24:]


def compare_objects(a, b):
    """(kernels, [messages about kernels that differ]) of two code objects"""
    bad = []
    for s in sorted(set(a.meta) ^ set(b.meta)):
        bad.append(f'{s}: only in the {"parent" if s in a.meta else "branch"}')
    common = sorted(set(a.meta) & set(b.meta))
    whole = a.section('.text') == b.section('.text') and a.section('.rodata') == b.section('.rodata')
    for s in common:
        if a.meta[s] != b.meta[s]:
            bad.append(f'{s}: metadata {dict(zip(META, a.meta[s]))} -> {dict(zip(META, b.meta[s]))}')
        elif not whole and (a.symbol(s) is None or a.symbol(s) != b.symbol(s)):
            bad.append(f'{s}: machine code differs')
        elif not whole and descriptor(a, s) != descriptor(b, s):
            bad.append(f'{s}: kernel descriptor differs')
    return len(set(a.meta) | set(b.meta)), bad


def units(path, tmp):
    """name -> [code objects] of a csrc directory (per *.o) or of one file"""
    files = sorted(glob.glob(os.path.join(path, '*.o'))) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        sub = tempfile.mkdtemp(dir=tmp)
        out[os.path.basename(f)] = [CodeObject(co) for co in code_objects(f, sub)]
    return out


def main():
    parent, branch = sys.argv[1:3]
    total, differing = 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        A, B = units(parent, tmp), units(branch, tmp)
        for name in sorted(set(A) | set(B)):
            ca, cb = A.get(name, []), B.get(name, [])
            if len(ca) != len(cb):
                print(f'{name}: {len(ca)} code objects in the parent, {len(cb)} in the branch')
                differing += max(sum(len(c.meta) for c in ca), sum(len(c.meta) for c in cb), 1)
                continue
            for a, b in zip(ca, cb):
                n, bad = compare_objects(a, b)
                total += n
                differing += len(bad)
                for msg in bad:
                    print(f'{name}: {msg}')
    print(f'{total} kernels, {differing} differing')
    return 1 if differing else 0


if __name__ == '__main__':
    sys.exit(main())
