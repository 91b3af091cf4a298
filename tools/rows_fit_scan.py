"""Which instantiations of the widened nmf_rows (csrc/dn_generic.hip, wide-cohort build) keep their body free of scratch: the table
behind rows_fit<R, NSM, SAFE>.  Compiles the unit with -DDN_GEN_WIDE=1 -DDN_ROWS_FIT_ALL=1 (every R = 2, 3, 4, n = 2 .. 12, hot and
safe), disassembles the gfx950 code object and prints per instantiation: vector registers used, scratch stores, scratch loads, and
how many of them lie in the body -- a store after the entry block's saves of callee-saved registers or a load before the exit
blocks' restores (entry: up to the first branch; restores: loads of an offset that the entry block stored, with no other access to
that offset).  `fits` = no body access.  Run it after a compiler update and bring rows_fit into line.  No GPU needed.
usage: python tools/rows_fit_scan.py"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from degnorm_amd import build

B = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
with tempfile.TemporaryDirectory() as w:
    o, fb, co = (os.path.join(w, n) for n in ('w.o', 'w.fatbin', 'w.co'))
    build._run([build._hipcc()] + build.FLAGS + ['-DDN_GEN_NT=256', '-DDN_GEN_WIDE=1', '-DDN_ROWS_FIT_ALL=1', '-c',
                                                 os.path.join(build.CSRC, 'dn_generic.hip'), '-o', o])
    build._run([os.path.join(B, 'llvm-objcopy'), '--dump-section=.hip_fatbin=' + fb, o])
    build._run([os.path.join(B, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + fb,
                '--targets=hipv4-amdgcn-amd-amdhsa--' + build.ARCH, '--output=' + co])
    dis = build._run([os.path.join(B, 'llvm-objdump'), '-d', '--no-show-raw-insn', co])

body, cur = {}, None
for line in dis.splitlines():
    m = re.match(r'^[0-9a-f]+ <(.*)>:', line)
    if m:
        cur = m.group(1)
        body[cur] = []
    elif cur:
        body[cur].append(line.split('//')[0])
rows = {}
for name, ins in body.items():
    m = re.search(r'nmf_rowsILi(\d+)ELb([01])ELi(\d+)E', name)
    if not m:
        continue
    first_branch = next((i for i, l in enumerate(ins) if re.search(r'\bs_c?branch', l)), len(ins))
    acc = {}                                                   # offset -> [(index, 'st' | 'ld')]
    for i, l in enumerate(ins):
        k = re.search(r'scratch_(store|load)_\w+', l)
        if k:
            off = re.search(r'offset:(\d+)', l)
            acc.setdefault(int(off.group(1)) if off else 0, []).append((i, 'st' if k.group(1) == 'store' else 'ld'))
    n_st = sum(1 for v in acc.values() for a in v if a[1] == 'st')
    n_ld = sum(1 for v in acc.values() for a in v if a[1] == 'ld')
    in_body = 0
    for v in acc.values():
        stores = [a for a in v if a[1] == 'st']
        if len(stores) == 1 and stores[0][0] < first_branch:    # one save in the entry block, restores on the ways out
            continue
        in_body += len(v)
    regs = 1 + max([int(x) for l in ins for x in re.findall(r'\bv(\d+)\b', l)] +
                   [int(x) for l in ins for x in re.findall(r'v\[\d+:(\d+)\]', l)])
    rows[(int(m.group(3)), int(m.group(2)), int(m.group(1)))] = (regs, n_st, n_ld, in_body)
print('R safe  n  vgprs stores loads in_body fits')
for key in sorted(rows):
    print('%d %4d %3d %6d %6d %5d %7d %s' % (key + rows[key] + ('yes' if rows[key][3] == 0 else 'no',)))
