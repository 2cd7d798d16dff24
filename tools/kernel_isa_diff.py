#!/usr/bin/env python3
"""Compare the generated code of two builds kernel by kernel.

    make -C pointcloudcounterfactual_amd/csrc asm-<file>      (in both trees: writes csrc/_asm/<file>.s)
    tools/kernel_isa_diff.py OLD/_asm NEW/_asm

A kernel is keyed by its demangled name, so it may move between files.  Three things are compared per kernel:
the resource table the compiler prints behind the code (registers, scratch, LDS, occupancy, code length), the
.amdhsa_* descriptor block, and the instruction stream after normalising only local labels, symbol-name
suffixes that number a function inside its file, and directives (.loc, .file, .section, .p2align ...).
Exit status 0 iff no kernel differs and both sides hold the same kernels."""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys

INFO = re.compile(r'^\s*;\s*(codeLenInByte|NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize'
                  r'|SGPRBlocks|VGPRBlocks|NumSGPRsForWavesPerEU|NumVGPRsForWavesPerEU|WaveLimiterHint|MemoryBound):?\s*(.*)$')


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    for cand in ('/opt/rocm/llvm/bin/llvm-cxxfilt', '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'):
        if not tool and os.path.exists(cand):
            tool = cand
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, out))


def normalise(line):
    line = line.split(';', 1)[0].rstrip()                 # trailing comments
    line = re.sub(r'\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?', lambda m: '.L' + m.group(1) + (m.group(2) or ''), line)
    return re.sub(r'\s+', ' ', line).strip()


def parse(directory):
    """{demangled kernel name: (file, resources, descriptor lines, instruction lines)}"""
    kernels = {}
    for path in sorted(glob.glob(os.path.join(directory, '*.s'))):
        lines = open(path, errors='replace').read().split('\n')
        descs, i = {}, 0
        while i < len(lines):
            m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', lines[i])
            if m:
                j = i + 1
                while '.end_amdhsa_kernel' not in lines[j]:
                    j += 1
                descs[m.group(1)] = [normalise(x) for x in lines[i + 1:j]]
                i = j
            i += 1
        names = demangle(list(descs))
        for sym, desc in descs.items():
            start = next(k for k, x in enumerate(lines) if x.startswith(sym + ':'))
            body, res, k = [], {}, start + 1
            while not re.match(r'\s*\.Lfunc_end\d+:', lines[k]):
                t = normalise(lines[k])
                if t and not (t.startswith('.') and not t.endswith(':')):  # directives go, labels stay
                    body.append(t.replace(sym, '<kernel>'))
                k += 1
            # (the table follows a `.section .AMDGPU.csdata` line of its own; the next kernel begins with .text or its section)
            while k < len(lines) and not lines[k].startswith('\t.text') and not (lines[k].startswith('\t.section') and 'csdata' not in lines[k]):
                m = INFO.match(lines[k])
                if m:
                    res[m.group(1)] = m.group(2).strip()
                k += 1
            kernels[names[sym]] = (os.path.basename(path), res, desc, body)
    return kernels


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    differ = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            differ += 1
            print('ONLY IN %s: %s' % ('OLD' if name in old else 'NEW', name))
            continue
        (fo, ro, do, bo), (fn, rn, dn, bn) = old[name], new[name]
        what = [w for w, a, b in (('resources', ro, rn), ('descriptor', do, dn), ('instructions', bo, bn)) if a != b]
        if not what:
            continue
        differ += 1
        print('DIFFERS (%s): %s   [%s -> %s]' % (', '.join(what), name, fo, fn))
        for key in sorted(set(ro) | set(rn)):
            if ro.get(key) != rn.get(key):
                print('    %s: %s -> %s' % (key, ro.get(key), rn.get(key)))
        for a, b in ((do, dn), (bo, bn)):
            for d in list(difflib.unified_diff(a, b, 'old', 'new', n=1, lineterm=''))[:40]:
                print('    ' + d)
    moved = sum(1 for k in old if k in new and old[k][0] != new[k][0])
    print('%d kernels in OLD, %d in NEW, %d moved to another file: %d kernels differ' % (len(old), len(new), moved, differ))
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
