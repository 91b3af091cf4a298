"""
Static instruction count of ONE spill-tier column of the NMF pass, from the ISA of a -DDN_MARKS build (csrc/dn_kernels.hpp,
spill_tier).  tools/isa_regions.py prices a whole region (prologue and loop counted together); this tool isolates the column loop
inside the spill_tier / spill_tier_b regions of every nmf() body that carries a spill tier and lists, per trip of that loop: vector,
scalar and memory instructions, the state accesses by width, the selects (v_cndmask) and the scratch accesses; and, per body, the
scratch accesses and scalar-spill lane writes of the whole T loop (iter_begin .. solved).
usage: python tools/spill_column_isa.py <p> [<file.s> <nt> ...]     without files: compiles pair, 128 and wide builds itself
"""
import os, re, subprocess, sys, tempfile
from collections import Counter
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CADENCE = 4.08          # cycles per issue slot at one wave per SIMD (tools/ubench/instr_cost.hip)


def compile_marks(p, nt, pair, out):
    from degnorm_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.sched_flags(p) + build.EXTRA + ['-DDN_P=%d' % p, '-DDN_NT=%d' % nt, '-DDN_MARKS'] + \
          (['-DDN_PAIR=1'] if pair else []) + ['-S', '--cuda-device-only', os.path.join(ROOT, 'degnorm_amd', 'csrc', 'dn_inst.hip'), '-o', out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out


def _ops(lines):
    """(opcode, text) of every instruction line"""
    r = []
    for l in lines:
        t = l.strip()
        if not l.startswith('\t') or not t or t[0] in '.;':
            continue
        r.append((t.split()[0], t.split(';')[0].strip()))
    return r


def _column_loop(region, anchor):
    """the lines of the column loop of a region: the smallest span label .. last backward branch to it that holds an `anchor` store
    (the loop's blocks are not laid out in source order: the prefetch block usually follows the header it branches back to)"""
    best = None
    for i, l in enumerate(region):
        m = re.match(r'^(\.LBB\w+):', l)
        if not m:
            continue
        back = [j for j in range(i + 1, len(region)) if re.match(r's_c?branch\w*\s+' + re.escape(m.group(1)) + r'$', region[j].split(';')[0].strip())]
        if back and any(anchor in x for x in region[i:back[-1]]) and (best is None or back[-1] - i < best[1] - best[0]):
            best = (i, back[-1])
    return region[best[0]:best[1] + 1] if best else None


def bodies(text, p, nt, safe=False):
    """One dict per nmf() body of nmf_call<p, nt, safe> (in code order): 't_loop' = scratch / lane-spill lines between iter_begin and
    solved, 'columns' = {region name: counts of one trip of the spill tier's column loop} (empty for the on-chip body)."""
    fn = text[text.index('_ZN2dn8nmf_callILi%dELi%dELb%dE' % (p, nt, int(safe))):]
    lines = fn[:fn.index('.Lfunc_end')].split('\n')
    starts = [i for i, l in enumerate(lines) if 'DN_MARK iter_begin' in l]
    res = []
    for b, lo in enumerate(starts):
        hi = starts[b + 1] if b + 1 < len(starts) else len(lines)
        marks = [(i, re.search(r'DN_MARK (\w+)', lines[i]).group(1)) for i in range(lo, hi) if 'DN_MARK' in lines[i]]
        end = next((i for i, m in marks if m == 'solved'), hi)
        t_ops = _ops(lines[lo:end])
        body = {'t_loop_scratch': [t for o, t in t_ops if o.startswith('scratch_')],
                't_loop_lane_spill': [t for o, t in t_ops if o == 'v_writelane_b32'],       # a scalar spill WRITES a lane (v_readlane alone also serves broadcasts)
                'columns': {}}
        for q, (i, m) in enumerate(marks):
            if not m.startswith(('spill_tier', 'lds_tier')):
                continue
            region = lines[i + 1:marks[q + 1][0]]
            loop = _column_loop(region, 'global_store' if m.startswith('spill') else 'ds_write')
            if loop is None:
                continue
            ops = _ops(loop)
            c = Counter()
            for o, t in ops:
                if o.startswith('scratch_'): c['scratch'] += 1
                elif o.startswith(('global_', 'flat_', 'buffer_')): c['memory'] += 1
                elif o.startswith('ds_'): c['lds'] += 1
                elif o.startswith('v_'): c['vector'] += 1
                else: c['scalar'] += 1
                if o.startswith('v_cndmask'): c['cndmask'] += 1
                if o.startswith('v_mov') or o.startswith('v_accvgpr'): c['moves'] += 1
                m2 = re.match(r'global_(load|store)_dword(x\d)?$', o)
                if m2:
                    # the counts are fp32 loads from their own base; state accesses are 64- or 128-bit
                    c['%s_%d' % (m2.group(1), {None: 32, 'x2': 64, 'x3': 96, 'x4': 128}[m2.group(2)])] += 1
            c['slots'] = len(ops)
            c['region_cndmask'] = sum(o.startswith('v_cndmask') for o, t in _ops(region))
            body['columns'][m] = c
        res.append(body)
    return res


def report(text, p, nt, label):
    print('nmf_call<%d,%d> (%s)' % (p, nt, label))
    for b, body in enumerate(bodies(text, p, nt)):
        print('  body %d: T loop (iter_begin .. solved): %d scratch accesses, %d scalar-spill lane writes (v_writelane)'
              % (b, len(body['t_loop_scratch']), len(body['t_loop_lane_spill'])))
        for name, c in body['columns'].items():
            print('    %-13s per column: %3d slots = vector %3d (moves %2d, cndmask %2d) + scalar %2d + memory %2d + lds %d, scratch %d'
                  '  ~%4.0f cycles at %.2f;  loads 32b %d 64b %d 96b %d 128b %d, stores 64b %d 128b %d;  cndmask in whole region %d'
                  % (name, c['slots'], c['vector'], c['moves'], c['cndmask'], c['scalar'], c['memory'], c['lds'], c['scratch'], c['slots'] * CADENCE, CADENCE,
                     c['load_32'], c['load_64'], c['load_96'], c['load_128'], c['store_64'], c['store_128'], c['region_cndmask']))


def main():
    p = int(sys.argv[1])
    if len(sys.argv) > 2:
        for f, nt in zip(sys.argv[2::2], sys.argv[3::2]):
            report(open(f).read(), p, int(nt), os.path.basename(f))
        return
    from degnorm_amd import build
    d = tempfile.mkdtemp()
    for nt, pair in ((64, True), (128, False), (build.WIDE_NT, False)):
        report(open(compile_marks(p, nt, pair, os.path.join(d, 'k%d.s' % nt))).read(), p, nt, 'pair build' if pair else 'product flags')


if __name__ == '__main__':
    main()
