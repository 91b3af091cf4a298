"""
Static guards for the partial register-tier body of the NMF pass (csrc/dn_kernels.hpp: nmf_body<P, NT, true, false>, the body of a call
with fewer columns than the register tier holds), on the ISA of -DDN_MARKS builds of the three p = 10 units
compiled for gfx950 with the flags build.py uses -- no GPU needed.  The body pads its tier to whole rounds at the cold start and walks
the rounds the gene reaches unmasked, so each copy of its tier must be the full tier's code: 161 vector instructions per column, no
write to the exec mask (one uniform branch per round leaves the chain instead), and nothing in its T loop goes through scratch.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 10
COLUMN = 161                                                              # vector instructions of a register-tier column at p = 10 (raw-unit pass)
RT = min(12, 256 // (2 * P + (P + 1) // 2))                               # dn_kernels.hpp rt_cols<P, X16 = true>: columns per lane


def _variants():
    from degnorm_amd import build
    return [(64, True), (128, False), (build.WIDE_NT, False)]           # pair build, narrow class, wide class


@pytest.fixture(scope='module')
def marks_isa(tmp_path_factory):
    from degnorm_amd import build
    d = tmp_path_factory.mktemp('partial_isa')
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
    """The nmf() bodies of nmf_call<10, nt, false> in code order (on-chip, full tier, partial tier, counts beyond 16 bits), each as
    (instructions of the T loop, {name of a register-tier mark: instructions from it to the next mark})."""
    fn = text[text.index('_ZN2dn8nmf_callILi{0}ELi{1}ELb0E'.format(P, nt)):]
    lines = fn[:fn.index('.Lfunc_end')].split('\n')
    starts = [i for i, l in enumerate(lines) if 'DN_MARK iter_begin' in l]
    res = []
    for b, lo in enumerate(starts):
        body = lines[lo:starts[b + 1] if b + 1 < len(starts) else len(lines)]
        marks = [(i, re.search(r'DN_MARK (\w+)', l).group(1)) for i, l in enumerate(body) if 'DN_MARK' in l]
        end = next(i for i, m in marks if m == 'solved')
        tiers = {}
        for q, (i, name) in enumerate(marks):
            if name in ('reg_tier', 'reg_tier_b') and i < end:
                assert name not in tiers
                tiers[name] = _instructions(body[i + 1:marks[q + 1][0]])
        res.append((_instructions(body[:end]), tiers))
    return res


def _vector(ops, readlane=True):
    return sum(1 for t in ops if t.startswith('v_') and (readlane or not t.startswith('v_readlane')))


def _writes_exec(t):
    op, _, args = t.partition(' ')
    dst = args.split(',')[0].strip()
    return 'saveexec' in op or op.startswith('v_cmpx') or dst in ('exec', 'exec_lo', 'exec_hi')


@pytest.mark.parametrize('nt', [v[0] for v in _variants()])
def test_partial_body_walks_its_padded_tier_unmasked(marks_isa, nt):
    bodies = _bodies(marks_isa[nt], nt)
    assert len(bodies) == 4
    t_loop, tiers = bodies[2]                                             # the partial body: third in code order
    assert not [t for t in t_loop if t.startswith('scratch_')], 'scratch access in the partial body\'s T loop (NT = %d)' % nt
    assert not [t for t in t_loop if t.startswith('v_writelane')], 'scalar spill in the partial body\'s T loop (NT = %d)' % nt
    assert tiers                                                          # one copy per walking direction that carries one
    for name, ops in tiers.items():
        # v_readlane: the round count comes back from a lane of a vector register once per round, not part of a column
        assert _vector(ops, readlane=False) == RT * COLUMN, (name, _vector(ops, readlane=False))
        assert not [t for t in ops if _writes_exec(t)], (name, [t for t in ops if _writes_exec(t)])
        assert sum(1 for t in ops if t.startswith('v_accvgpr')) == RT * (2 * 2 * P + (P + 1) // 2)      # state read and written, counts read


@pytest.mark.parametrize('nt', [v[0] for v in _variants()])
def test_other_bodies_keep_their_register_tiers(marks_isa, nt):
    """The partial body is changed in place: the on-chip and the full body keep the straight-line tier of RT x 161 vector instructions
    (v_readlane included: they have none), the body for counts beyond 16 bits its masked tier that reads the counts from memory."""
    bodies = _bodies(marks_isa[nt], nt)
    assert {k: _vector(v) for k, v in bodies[0][1].items()} == {'reg_tier': RT * COLUMN}
    assert {k: _vector(v) for k, v in bodies[1][1].items()} == {'reg_tier': RT * COLUMN, 'reg_tier_b': RT * COLUMN}
    assert {k: _vector(v) for k, v in bodies[3][1].items()} == {'reg_tier': 201, 'reg_tier_b': 146}
