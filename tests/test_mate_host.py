"""
Pairing by FLAG without a GPU: bam.mate_rows, the host build of the passes of csrc/dn_pair.hip with the coordinate chunk,
against a numpy restatement (a stable np.lexsort on padded names and the two coordinates), element for element; the paired /
single-end decision of the three pairing modes on small files through the host framing; and the argument checks.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _flag_cases as fc                                       # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

F, L = 0x41, 0x81

CASES = [
    ('n0', []),
    ('n1', [(b'b', 5, 9, F)]),
    ('n2', [(b'b', 9, 5, L), (b'b', 5, 9, F)]),
    ('n3', [(b'b', 9, 5, L), (b'a', 1, 2, F), (b'b', 5, 9, F)]),
    ('prefixes', [(b'r10', 1, 2, F), (b'r1', 1, 2, F), (b'r1.a', 2, 1, L), (b'r', 7, 7, F), (b'r1', 2, 1, L), (b'', 3, 4, F), (b'r10', 2, 1, L),
                  (b'', 4, 3, L), (b'abcdefghz', 3, 4, F), (b'abcdefgh', 3, 4, F), (b'abcdefghz', 4, 3, L)]),
    ('two_loci', [(b't', 100, 300, F), (b't', 5000, 5200, F), (b't', 300, 100, L), (b't', 5200, 5000, L), (b't', 100, 301, F)]),
    ('pos_first_is_pos_last', [(b's', 40, 40, F), (b's', 40, 40, L), (b's', 40, 41, L), (b's', 41, 40, F)]),
    ('no_mate_position', [(b'u', 7, -1, F), (b'u', 7, -1, L), (b'u', 0, -1, L), (b'v', 2 ** 31 - 1, -1, F), (b'u', 0, -1, F)]),
]


def _check(names, pos, next_pos, flag, what):
    order_e, pair_id_e, n_ids_e = fc.restate(names, pos, next_pos, flag)
    for given in (fc.padded(names), list(names)):              # an S array, and a list of bytes
        order, pair_id, n_ids = bam.mate_rows(given, pos, next_pos, flag)
        assert order.dtype == np.int32 and pair_id.dtype == np.int32 and len(order) == len(pair_id) == len(names), what
        assert np.array_equal(order, order_e), what
        assert np.array_equal(pair_id, pair_id_e), what
        assert n_ids == n_ids_e, what


@pytest.mark.parametrize('what,case', CASES, ids=[c[0] for c in CASES])
def test_mate_rows_equals_numpy(what, case):
    names, pos, next_pos, flag = ([r[k] for r in case] for k in range(4))
    _check(names, pos, next_pos, flag, what)


def test_the_contract_on_a_case_read_by_hand():
    """Ties in file order, a prefix first, -1 before 0, and two loci of one name apart."""
    order, pair_id, n_ids = bam.mate_rows([b't', b't', b'r1', b't', b'r', b't', b't'], [300, 100, 4, 5000, 4, 100, 5200],
                                          [100, 300, -1, 5200, -1, 300, 5000], [L, F, F, F, L, F, L])
    # keys: (r, 0, 5) | (r1, 5, 0) | (t, 101, 301) x 3 in file order | (t, 5001, 5201) x 2
    assert order.tolist() == [4, 2, 0, 1, 5, 3, 6] and pair_id.tolist() == [0, 1, 2, 2, 2, 3, 3] and n_ids == 4


def test_mate_rows_5000_seeded_rows():
    r = fc.random_mates(5000, 60, seed=11)
    names = [q.encode() for q in r.qname]
    _, _, n_ids = fc.restate(names, r.pos.values, r.next_pos.values, r.flag.values)
    assert 1000 < n_ids < 4500 and len(set(len(k) for k in names)) > 8         # keys that repeat, names around the 8-byte chunk
    _check(names, r.pos.values, r.next_pos.values, r.flag.values, 'seeded')


def test_mate_rows_checks_its_arguments():
    with pytest.raises(ValueError, match='one entry per row'):
        bam.mate_rows([b'a', b'b'], [1], [2, 3], [F, L])


# --- the paired / single-end decision ------------------------------------------------------------------------------------

def _file(tmp_path, name, records):
    p = str(tmp_path / (name + '.bam'))
    fc.write_bam(p, [('c', 2000)], fc.rows(records))
    return p


@pytest.fixture()
def files(tmp_path):
    flagged = [('g{0}'.format(i // 2), 100 + i, '20M', (F if i % 2 == 0 else L), 100 + (i ^ 1)) for i in range(20)]
    named = [('g{0}.{1}'.format(i // 2, 1 + i % 2), 100 + i, '20M', 0, 100 + i) for i in range(20)]
    single = [('q{0}'.format(i), 100 + i, '20M', 0x10 * (i % 2), 0, -1) for i in range(20)]
    # the one paired record lies behind the first 301: the file counts as single-end
    late = [('q{0}'.format(i), 100 + i, '20M', 0, 0, -1) for i in range(301)] + [('late', 500, '20M', F, 600)]
    both = [('g{0}.{1}'.format(i // 2, 1 + i % 2), 100 + i, '20M', (F if i % 2 == 0 else L), 100 + (i ^ 1)) for i in range(20)]
    return {k: _file(tmp_path, k, v) for k, v in dict(flagged=flagged, named=named, single=single, late=late, both=both).items()}


@pytest.mark.parametrize('pairing,expect', [
    ('name', dict(flagged=(False, 'name'), named=(True, 'name'), single=(False, 'name'), late=(False, 'name'), both=(True, 'name'))),
    ('flag', dict(flagged=(True, 'flag'), named=(False, 'flag'), single=(False, 'flag'), late=(False, 'flag'), both=(True, 'flag'))),
    ('auto', dict(flagged=(True, 'flag'), named=(True, 'name'), single=(False, 'name'), late=(False, 'name'), both=(True, 'name'))),
])
def test_paired_decision_of_the_three_modes(pairing, expect, files, tmp_path):
    for name, (paired, rule) in expect.items():
        proc = bam.NativeBamReadsProcessor(files[name], files[name] + '.bai', output_dir=str(tmp_path / 'out'), verbose=False, pairing=pairing)
        assert (proc.paired, proc.pairing_rule, proc.pairing) == (paired, rule, pairing), name
    default = bam.NativeBamReadsProcessor(files['flagged'], files['flagged'] + '.bai', output_dir=str(tmp_path / 'out'), verbose=False)
    assert (default.paired, default.pairing, default.pairing_rule) == (False, 'name', 'name')


# --- the argument checks ---------------------------------------------------------------------------------------------------

BAD = [(dict(pairing='bogus'), "pairing must be 'name' or 'flag' or 'auto', not 'bogus'"),
       (dict(exclude_flags=-1), r'exclude_flags must be an integer in 0 \.\. 65535, not -1'),
       (dict(exclude_flags=0x10000), r'exclude_flags must be an integer in 0 \.\. 65535, not 65536'),
       (dict(require_flags='0x2'), r"require_flags must be an integer in 0 \.\. 65535, not '0x2'"),
       (dict(min_mapq=256), r'min_mapq must be an integer in 0 \.\. 255, not 256'),
       (dict(min_mapq=1.5), r'min_mapq must be an integer in 0 \.\. 255, not 1\.5'),
       (dict(min_mapq=True), r'min_mapq must be an integer in 0 \.\. 255, not True')]


@pytest.mark.parametrize('kw,text', BAD, ids=[sorted(k)[0] + str(i) for i, (k, _) in enumerate(BAD)])
def test_bad_options_are_refused_before_any_file_is_opened(kw, text, tmp_path):
    missing = str(tmp_path / 'missing.bam')                    # no such file: the option is what is refused
    with pytest.raises(ValueError, match=text):
        bam.NativeBamReadsProcessor(missing, missing + '.bai', **kw)
    from degnorm_amd import pipeline
    with pytest.raises(ValueError, match=text):
        pipeline.prepare_inputs([missing], [missing + '.bai'], missing, str(tmp_path), **kw)
    with pytest.raises(ValueError, match=text):
        pipeline.run_pipeline([missing], [missing + '.bai'], missing, str(tmp_path), **kw)


def test_options_reach_run_pipeline_from_the_command_line(tmp_path, monkeypatch):
    from degnorm_amd import __main__ as cli
    from degnorm_amd import pipeline
    a = cli.argparser().parse_args([])
    assert (a.pair_by, a.exclude_flags, a.require_flags, a.min_mapq) == ('name', 0, 0, 0)
    for name in ('a.bam', 'a.bai', 'b.bam', 'b.bai', 'g.gtf'):
        (tmp_path / name).write_bytes(b'')
    seen = []
    monkeypatch.setattr(pipeline, 'run_pipeline', lambda *a, **kw: seen.append(kw))
    base = ['--bam-files', str(tmp_path / 'a.bam'), str(tmp_path / 'b.bam'), '-g', str(tmp_path / 'g.gtf')]
    assert cli.main(base + ['-o', str(tmp_path / 'o1'), '--pair-by', 'flag', '--exclude-flags', '0x904', '--min-mapq', '10']) == 0
    assert cli.main(base + ['-o', str(tmp_path / 'o2'), '--pair-by', 'auto', '--require-flags', '2', '--exclude-flags', '1024']) == 0
    assert cli.main(base + ['-o', str(tmp_path / 'o3')]) == 0
    assert [(kw['pairing'], kw['exclude_flags'], kw['require_flags'], kw['min_mapq']) for kw in seen] == \
        [('flag', 0x904, 0, 10), ('auto', 1024, 2, 0), ('name', 0, 0, 0)]
    with pytest.raises(ValueError, match=r'min_mapq must be an integer in 0 \.\. 255, not 300'):
        cli.main(base + ['-o', str(tmp_path / 'o4'), '--min-mapq', '300'])
    assert not os.path.exists(str(tmp_path / 'o4'))
    with pytest.raises(SystemExit):
        cli.main(base + ['-o', str(tmp_path / 'o5'), '--exclude-flags', '0y4'])
