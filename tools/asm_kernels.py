#!/usr/bin/env python
"""Kernel-by-kernel identity of two device assemblies: the complement of tools/asm_identity.sh for a source that GAINED kernels, where the whole-file diff cannot be empty.

    tools/asm_identity.sh <parent tree> <result tree> OUT stitch.hip luma.hip misc_kernels.hip      (exits 1: the files differ; the stripped texts stay in OUT/a, OUT/b)
    python tools/asm_kernels.py OUT stitch luma misc_kernels                                        (one markdown table row per source)

Per kernel symbol the instruction text between its label and its .Lfunc_end, and its .amdhsa_kernel descriptor block (registers, LDS, scratch, kernarg size), are compared
after the function's ordinal is taken out of the local labels (.LBB<n>_<k>, .Lfunc_end<n>: inserting a kernel renumbers the ones behind it).  Exits 1 when a kernel
both sides have differs, or when the parent has a kernel the result lost."""
import hashlib
import os
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read().splitlines()
    out, cur, name = {}, None, None
    for line in text:
        m = re.match(r'^(_Z\w+):', line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r'^\.Lfunc_end\d+:', line):
                out[name] = ['\n'.join(cur), '']
                cur = None
            else:
                cur.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s*;.*$', '', line)))          # (a trailing comment names a block by the function's ordinal too)
    desc = None
    for line in text:
        m = re.match(r'^\s*\.amdhsa_kernel (\S+)', line)
        if m:
            name, desc = m.group(1), []
        elif desc is not None:
            if '.end_amdhsa_kernel' in line:
                if name in out:
                    out[name][1] = '\n'.join(desc)
                desc = None
            else:
                desc.append(line.strip())
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(['c++filt'], input='\n'.join(names) + '\n', capture_output=True, text=True).stdout.splitlines()
    clean = lambda n: re.sub(r'\(.*$', '', n.replace('void ', '').replace('(anonymous namespace)::', ''))
    return {k: clean(v) or k for k, v in zip(names, r)}


def main():
    out, bad = sys.argv[1], 0
    print('| source | kernels in the parent | identical in the result (code and descriptor) | differing | lost | new in the result |')
    print('|---|---|---|---|---|---|')
    for stem in sys.argv[2:]:
        a, b = kernels(os.path.join(out, 'a', stem + '.s')), kernels(os.path.join(out, 'b', stem + '.s'))
        same = [k for k in a if k in b and a[k] == b[k]]
        diff = [k for k in a if k in b and a[k] != b[k]]
        lost = [k for k in a if k not in b]
        new = [k for k in b if k not in a]
        names = demangle(diff + lost)
        print('| {}.hip | {} | {} | {} | {} | {} |'.format(stem, len(a), len(same), ', '.join(names[k] for k in diff) or 0, ', '.join(names[k] for k in lost) or 0, len(new)))
        bad |= bool(diff or lost)
    h = hashlib.sha256()
    for stem in sys.argv[2:]:
        for k, v in sorted(kernels(os.path.join(out, 'a', stem + '.s')).items()):
            h.update((k + v[0] + v[1]).encode())
    print('\nsha256 over the parent\'s kernels (normalised text and descriptors): ' + h.hexdigest())
    return bad


if __name__ == '__main__':
    sys.exit(main())
