#!/usr/bin/env python3
"""Per-kernel resource table of HIP sources, from their gfx950 assembly; needs no GPU.

    tools/kernel_stats.py field.hip render_infer.hip            this tree
    tools/kernel_stats.py --against ../parent field.hip ...     rows that differ between another checkout and this tree

Compiles with build.py's own flags (the per-file ones included) plus -S --cuda-device-only and prints, per kernel: instruction
count, .amdhsa_next_free_vgpr, .amdhsa_accum_offset (where the AGPRs start), scratch and static LDS bytes, and the waves per
SIMD those registers allow (512 registers per lane in granules of 8, at most 8 waves).  --keep DIR keeps the .s files, named
<tree>_<file>.s, for a `diff`.  It counts instructions and reports metadata; it does not look for particular instructions.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfstyle_amd import build  # noqa: E402

FIELDS = ('next_free_vgpr', 'accum_offset', 'private_segment_fixed_size', 'group_segment_fixed_size')
HEAD = ('instr', 'vgpr', 'agpr@', 'scratch', 'lds', 'waves')


def stats(tree, name, out):
    """{kernel: (instructions, vgpr, accum_offset, scratch, lds, waves)} of <tree>/nerfstyle_amd/csrc/<name>"""
    src = os.path.join(tree, 'nerfstyle_amd', 'csrc', os.path.basename(name))
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA_FLAGS.get(os.path.basename(name), []) + ['-S', '--cuda-device-only', src, '-o', out]
    subprocess.run(cmd, check=True)         # the compiler's warnings and errors go to the terminal
    text = open(out).read()
    res = {}
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', text, re.M | re.S):
        kern, meta = m.group(1), m.group(2)
        body = re.search(r'^%s:.*?\n(.*?)^\.Lfunc_end' % re.escape(kern), text, re.M | re.S).group(1)
        ninstr = len(re.findall(r'^\t[a-z]\w*', body, re.M))          # directives start with '.', labels and comments in column 0
        v = [int(re.search(r'\.amdhsa_%s (\d+)' % f, meta).group(1)) for f in FIELDS]
        res[kern] = (ninstr, *v, min(8, 512 // ((v[0] + 7) // 8 * 8)))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('files', nargs='+', help='names of .hip files under nerfstyle_amd/csrc')
    ap.add_argument('--against', metavar='TREE', help='another checkout: print only the rows that differ from it')
    ap.add_argument('--keep', metavar='DIR', help='keep the assembly files here')
    args = ap.parse_args()
    keep = args.keep or tempfile.mkdtemp(prefix='kernel_stats_')
    os.makedirs(keep, exist_ok=True)
    ndiff = 0
    for f in args.files:
        stem = os.path.basename(f).replace('.hip', '')
        new = stats(ROOT, f, os.path.join(keep, 'this_%s.s' % stem))
        old = stats(args.against, f, os.path.join(keep, 'other_%s.s' % stem)) if args.against else None
        print('%s: %d kernels  (%s)' % (f, len(new), ' '.join(HEAD)))
        for k in sorted(set(new) | set(old or {})):
            if old is None:
                print('  %-100s %s' % (k, ' '.join('%6d' % x for x in new[k])))
            elif old.get(k) != new.get(k):
                ndiff += 1
                print('  %s\n    other %s\n    this  %s' % (k, old.get(k), new.get(k)))
    if args.against:
        print('%d rows differ' % ndiff)
    return 1 if ndiff else 0


if __name__ == '__main__':
    sys.exit(main())
