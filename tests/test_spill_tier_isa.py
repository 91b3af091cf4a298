"""
Static guards for the spill tier of the NMF pass (csrc/dn_kernels.hpp, spill_tier), on the ISA of -DDN_MARKS
builds of the p = 10 units compiled for gfx950 with the flags build.py uses -- no GPU needed.  At one wave per SIMD every instruction
of the column loop is an issue slot, so what the loop must NOT contain is checked instruction by instruction.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 10
PS = P + (P & 1)


def _variants():
    from degnorm_amd import build
    return [(64, True), (128, False), (build.WIDE_NT, False)]           # pair build, narrow class, wide class


@pytest.fixture(scope='module')
def marks_isa(tmp_path_factory):
    """ISA with region marks of the three p = 10 units, compiled like the tier_isa fixture of test_host.py plus -DDN_MARKS."""
    from degnorm_amd import build
    d = tmp_path_factory.mktemp('spill_isa')
    src = os.path.join(ROOT, 'degnorm_amd', 'csrc', 'dn_inst.hip')

    def compile_one(v):
        nt, pair = v
        out = str(d / 'marks_p{0}_{1}.s'.format(P, 'pair' if pair else nt))
        cmd = [build._hipcc()] + build.FLAGS + build.sched_flags(P) + build.EXTRA + ['-DDN_P={0}'.format(P), '-DDN_NT={0}'.format(nt), '-DDN_MARKS'] + \
              (['-DDN_PAIR=1'] if pair else []) + ['-S', '--cuda-device-only', src, '-o', out]
        subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        return nt, open(out).read()
    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(ex.map(compile_one, _variants()))


def _instructions(lines):
    out = []
    for l in lines:
        t = l.strip()
        if l.startswith('\t') and t and t[0] not in '.;':
            out.append(t.split(';')[0].strip())
    return out


def _bodies(text, nt):
    """The nmf() bodies of nmf_call<10, nt, false>, in code order: (lines of the body, its marks as (line, name))."""
    fn = text[text.index('_ZN2dn8nmf_callILi{0}ELi{1}ELb0E'.format(P, nt)):]
    lines = fn[:fn.index('.Lfunc_end')].split('\n')
    starts = [i for i, l in enumerate(lines) if 'DN_MARK iter_begin' in l]
    res = []
    for b, lo in enumerate(starts):
        hi = starts[b + 1] if b + 1 < len(starts) else len(lines)
        body = lines[lo:hi]
        res.append((body, [(i, re.search(r'DN_MARK (\w+)', l).group(1)) for i, l in enumerate(body) if 'DN_MARK' in l]))
    return res


def _column_loop(region):
    """(first, last) line of the spill tier's column loop inside a region: the smallest span from a label to the LAST backward branch
    to it that contains a global store (the blocks of a loop are not laid out in source order)."""
    best = None
    for i, l in enumerate(region):
        m = re.match(r'^(\.LBB\w+):', l)
        if not m:
            continue
        back = [j for j in range(i + 1, len(region)) if re.match(r's_c?branch\w*\s+' + re.escape(m.group(1)) + r'$', region[j].split(';')[0].strip())]
        if back and any('global_store' in x for x in region[i:back[-1]]) and (best is None or back[-1] - i < best[1] - best[0]):
            best = (i, back[-1])
    assert best is not None, 'no column loop in the spill tier region'
    return best


@pytest.mark.parametrize('nt', [v[0] for v in _variants()])
def test_spill_tier_column_is_on_its_instruction_diet(marks_isa, nt):
    """
    Every p = 10 body of nmf_call<10, NT> (pair build NT = 64, narrow 128, wide 256 unless DN_WIDE_NT says otherwise):
      * no scratch access and no scalar-spill lane write (v_writelane) anywhere in the T loop, iter_begin .. solved -- for the on-chip
        body too, whose pass test_host.py already guards;
    and every body that carries a spill tier, in both walking directions (spill_tier / spill_tier_b):
      * a column moves its state with exactly PS / 2 loads and PS / 2 stores of 128 bits from ONE address each (immediate offsets
        (q - PS / 4) * 1 024, the planes of spill_col) and with no 64-bit state access; the only other memory instructions of the
        loop are the column's three count loads;
      * no v_cndmask from the region's mark to the end of its column loop: the state is read unconditionally (the cold start wrote
        it) and the prefetch index is clamped with v_min / v_max.  (What the scheduler places between the loop's end and the next
        mark belongs to the reduction that follows the pass: its first steps select between accumulators.)
    """
    bodies = _bodies(marks_isa[nt], nt)
    assert len(bodies) == 4                                               # on-chip, full register tier, partial, counts beyond 16 bits
    with_spill = 0
    offsets = sorted((q - PS // 4) * 1024 for q in range(PS // 2))
    for body, marks in bodies:
        end = next(i for i, m in marks if m == 'solved')
        t_loop = _instructions(body[:end])
        assert not [t for t in t_loop if t.startswith('scratch_')], 'scratch access in a T loop (NT = %d)' % nt
        assert not [t for t in t_loop if t.startswith('v_writelane')], 'scalar spill in a T loop (NT = %d)' % nt
        for q, (i, name) in enumerate(marks):
            if name not in ('spill_tier', 'spill_tier_b'):
                continue
            with_spill += 1
            region = body[i + 1:marks[q + 1][0]]
            lo, hi = _column_loop(region)
            assert not [t for t in _instructions(region[:hi + 1]) if t.startswith('v_cndmask')]
            loop = _instructions(region[lo:hi + 1])
            mem = [t for t in loop if t.startswith(('global_', 'flat_', 'buffer_', 'scratch_'))]
            stores = [t for t in mem if 'store' in t]
            loads = [t for t in mem if 'load' in t]
            assert len(stores) == PS // 2 and all(t.startswith('global_store_dwordx4 ') for t in stores), stores
            assert len(set(t.split()[1] for t in stores)) == 1            # one address register pair
            off = lambda t: int(re.search(r'offset:(-?\d+)', t).group(1)) if 'offset:' in t else 0
            assert sorted(off(t) for t in stores) == offsets
            # the loads: the column's P fp32 counts (128-bit pieces from offset 0, the rest 64- / 32-bit) and the PS / 2 planes of the
            # state, all of them 128 bits wide (registers are reused inside the loop, so the two groups are told apart by offset)
            count_offsets = list(range(0, 4 * P, 16))
            wide = sorted(off(t) for t in loads if t.startswith('global_load_dwordx4 '))
            assert wide == sorted(offsets + [o for o in count_offsets if o + 16 <= 4 * P]), loads
            narrow = [t for t in loads if not t.startswith('global_load_dwordx4 ')]
            assert all(off(t) in count_offsets for t in narrow) and len(narrow) == len(loads) - len(wide) <= 2, narrow
            assert len(mem) == PS + 3
    assert with_spill == 6                                                # three bodies x two directions
