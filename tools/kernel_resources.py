"""The compiler's per-kernel resource report of one or more sources of two checkouts, side by side: SGPRs, VGPRs, scratch bytes per
lane, occupancy (waves per SIMD) and LDS bytes per block, from `-Rpass-analysis=kernel-resource-usage` on top of the build's own flags
(efgh_amd/build.py).  Nothing is linked or run; it needs hipcc and no GPU.

    python tools/kernel_resources.py --parent DIR [--rename OLD=NEW ...] lattice.hip prep.hip

`--rename OLD=NEW` lists the parent's kernel OLD against this checkout's NEW (a kernel that was replaced by a template instance);
names are the demangled ones with the `(anonymous namespace)::` and the argument list dropped.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from efgh_amd import build as B  # noqa: E402

FIELDS = (('SGPRs', 'TotalSGPRs'), ('VGPRs', 'VGPRs'), ('scratch', r'ScratchSize \[bytes/lane\]'), ('occupancy', r'Occupancy \[waves/SIMD\]'),
          ('LDS', r'LDS Size \[bytes/block\]'))


def short(mangled):
    name = subprocess.run(['c++filt', mangled], capture_output=True, text=True).stdout.strip() or mangled
    name = name.replace('(anonymous namespace)::', '')
    name = re.sub(r'^void ', '', name)
    depth, out = 0, ''
    for ch in name:                                           # drop the argument list: the first '(' outside template brackets
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            break
        out += ch
    return out


def report(root, src):
    """{kernel: (SGPRs, VGPRs, scratch, occupancy, LDS)} of root/efgh_amd/csrc/src, in the order of the report"""
    path = os.path.join(root, 'efgh_amd', 'csrc', src)
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'hip'] + B.COMMON + B.EXTRA.get(src, []) + [
        '-Rpass-analysis=kernel-resource-usage', '-c', path, '-o', os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(p.stderr)
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = short(m.group(1))
            out[cur] = {}
            continue
        for key, pat in FIELDS:
            m = re.search(r'remark: .*\s' + pat + r': (\d+)', line)
            if m and cur is not None:
                out[cur][key] = int(m.group(1))
    return {k: tuple(v.get(f) for f, _ in FIELDS) for k, v in out.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='checkout of the parent commit')
    ap.add_argument('--rename', action='append', default=[], help='OLD=NEW: the parent kernel OLD was replaced by NEW')
    ap.add_argument('sources', nargs='+')
    a = ap.parse_args()
    rename = dict(r.split('=', 1) for r in a.rename)
    head = '%-58s %-30s %-30s %s' % ('kernel (parent -> new)', 'parent S/V/scratch/occ/LDS', 'new S/V/scratch/occ/LDS', '')
    for src in a.sources:
        old, new = report(a.parent, src), report(ROOT, src)
        print('%s: %d kernels at the parent, %d now' % (src, len(old), len(new)))
        print(head)
        seen = set()
        for k, o in old.items():
            k2 = rename.get(k, k)
            if k2 not in new:                                 # (a rename meant for another source's kernel of the same name)
                k2 = k
            n = new.get(k2)
            seen.add(k2)
            label = k if k2 == k else '%s -> %s' % (k, k2)
            fmt = lambda t: '/'.join(str(x) for x in t) if t else 'gone'
            note = 'same' if n == o else ('' if n is None else 'differs')
            print('%-58s %-30s %-30s %s' % (label, fmt(o), fmt(n), note))
        for k, n in new.items():
            if k not in seen:
                print('%-58s %-30s %-30s %s' % (k, 'new', '/'.join(str(x) for x in n), ''))
        print()


if __name__ == '__main__':
    main()
