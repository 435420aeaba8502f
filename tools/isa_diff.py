#!/usr/bin/env python
"""Compare the gfx950 machine code of two builds kernel by kernel: the acceptance test of a refactor under csrc/.  Compile both
trees into two directories with the recipe of tools/isa_scan.py, then
    python tools/isa_diff.py /tmp/isa/parent /tmp/isa/branch
For every kernel symbol it compares the instruction stream between its label and .Lfunc_end (comments dropped, the function
number of local labels normalised) and every .amdhsa_ value of its descriptor (VGPR / AGPR / SGPR counts, scratch, LDS, ...).
One line per kernel that is missing or differs, then a total; exit status 1 if anything differs.
"""
import re, sys
from isa_scan import kernels

SHOWN = ('next_free_vgpr', 'accum_offset', 'next_free_sgpr', 'private_segment_fixed_size', 'group_segment_fixed_size')


def split(body):
    """-> (normalised instruction lines, {descriptor field: value})"""
    code, desc, in_desc = [], {}, False
    for l in body:
        l = re.sub(r'\.L(BB|tmp|JTI|func_begin|func_end)\d+', r'.L\1', l.split(';')[0]).strip()
        if l.startswith('.amdhsa_kernel'): in_desc = True
        elif l.startswith('.end_amdhsa_kernel'): in_desc = False
        elif in_desc:
            k, _, v = l.partition(' ')
            desc[k[len('.amdhsa_'):]] = v.strip()
        elif l: code.append(l)
    return code, desc


def load(d):
    return {(stem, name): split(body) for stem, name, body in kernels(d)}


def main(a, b):
    A, B = load(a), load(b)
    differ = 0
    for key in sorted(set(A) | set(B)):
        tag = '%s %s' % key
        if key not in A or key not in B:
            print('%-8s %s' % ('ONLY-B' if key not in A else 'ONLY-A', tag)); differ += 1; continue
        (ca, da), (cb, db) = A[key], B[key]
        if ca == cb and da == db: continue
        differ += 1
        first = next((i for i, (x, y) in enumerate(zip(ca, cb)) if x != y), min(len(ca), len(cb)))
        regs = ' '.join('%s=%s/%s' % (k, da.get(k), db.get(k)) for k in SHOWN)
        what = 'DESC' if da != db else 'CODE'
        print('%-8s %s  insts=%d/%d first_diff=%d  %s' % (what, tag, len(ca), len(cb), first, regs))
        for k in sorted(set(da) | set(db)):
            if da.get(k) != db.get(k) and k not in SHOWN: print('           %s=%s/%s' % (k, da.get(k), db.get(k)))
    n = len(set(A) | set(B))
    print('symbols compared: %d (%d kernels, the rest device functions)   identical: %d   differing or missing: %d'
          % (n, sum(1 for k in set(A) | set(B) if (A.get(k) or B[k])[1]), n - differ, differ))
    return 1 if differ else 0


if __name__ == '__main__':
    if len(sys.argv) != 3: sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
