"""
GPU tests of pairing by FLAG and of the read filters (csrc/dn_pair.hip, k_bam_scan / k_bam_write / k_prefilter of
csrc/dn_reads.hip): DeviceRows(pairing='flag').pair against the numpy restatement of _flag_cases, element for element; a file
of a few thousand flag-style pairs against its twin under the name rule (names g<k>.1 / g<k>.2, pair='device'); hand-made
compositions of a key with stated counts; the filters against the existing path on the file without the filtered records; the
default on a standard file; the command line; and run to run.
"""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _flag_cases as fc                                       # noqa: E402
import _pair_cases as pc                                       # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
from test_gpu_bam import _files, _layout_case, _run, _same     # noqa: E402
from test_gpu_pair import _two_gene_case                       # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu

F, L = 0x41, 0x81


# --- the order and the ids of a store ------------------------------------------------------------------------------------

def _check_store(reads, what):
    """The rows through a FLAG-rule store: what it keeps is what was written, and its pairing is the restatement's."""
    reads = bf.sort_reads(reads)
    n = len(reads)
    rows = bam.DeviceRows(0, True, True, pairing='flag')
    try:
        if n:
            data, offs = fc.encode(reads)
            rows.append(data, offs)
        assert rows.info()[0] == n, what
        pos, _, _, _, name_beg, name_len, names = rows.fetch()
        flag, mapq, next_pos = rows.fetch_mates()
        nb = names.tobytes()
        got = [nb[b:b + k] for b, k in zip(name_beg.tolist(), name_len.tolist())]
        assert got == [q.encode() for q in reads.qname] and pos.tolist() == reads.pos.tolist(), what
        assert flag.tolist() == reads.flag.tolist() and mapq.tolist() == reads.mapq.tolist() and next_pos.tolist() == reads.next_pos.tolist(), what
        order_e, pair_id_e, n_ids_e = fc.restate(got, pos, next_pos, flag)
        order, pair_id, n_ids, ms = rows.pair(fetch=True)
        assert order.dtype == np.int32 and np.array_equal(order, order_e), what
        assert np.array_equal(pair_id, pair_id_e), what
        assert n_ids == n_ids_e and ms >= 0.0, what
        assert rows.pair()[:3] == (None, None, n_ids_e), what
        assert rows.dropped() == (0, 0, 0), what
        return n_ids
    finally:
        rows.close()


@pytest.mark.parametrize('n', [0, 1, 2, 3, 64, 65, 70001])
def test_sizes(n):
    """70 001 rows are more than one workgroup of the radix sort and, at 256 lanes, 274 blocks of the kernels."""
    n_ids = _check_store(fc.random_mates(n, max(n // 100, 3), seed=n), n)
    assert n_ids <= n and (n < 70001 or n // 4 < n_ids < n)    # keys that repeat and keys that do not


def test_one_name_at_3000_loci():
    """Every row has the same name: only the coordinate chunk tells the keys apart."""
    rng = np.random.default_rng(8)
    first = 1000 + rng.choice(200000, 3000, replace=False)
    last = first + rng.integers(-300, 300, 3000)
    r = pd.DataFrame({'ref': 0, 'qname': 'template', 'cigar': '20M', 'next_ref': 0, 'mapq': 60,
                      'pos': np.r_[first, last], 'next_pos': np.r_[last, first], 'flag': np.r_[np.full(3000, F), np.full(3000, L)]})
    assert _check_store(r, 'loci') == 3000


def test_a_store_that_does_not_pair_by_flag_keeps_no_mate_columns():
    rows = bam.DeviceRows(0, True, True)
    try:
        with pytest.raises(ValueError, match='dn_bam_rows_fetch_mates'):
            rows.fetch_mates()
    finally:
        rows.close()


# --- the twin ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def twins(tmp_path_factory):
    """~3 000 synthetic pairs written flag-style, and the same records renamed g<k>.1 / g<k>.2."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(31, 3000, True)
    flagged, twin = fc.flag_style(src, seed=5)
    d = tmp_path_factory.mktemp('twins')
    refs = [(chrom, chrom_len), ('other', chrom_len)]
    paths = []
    for name, df in (('flagged', flagged), ('twin', twin)):
        (d / name).mkdir()
        p = str(d / name / 's.bam')                            # one sample name: it heads a column of the counts
        written, _, _ = fc.write_bam(p, refs, df, straddle=True)
        paths.append(p)
    here = written[written.ref == 0]
    n_pairs, n_overlap, _ = pc.order_sensitive_pairs(here.qname.tolist(), here.pos.tolist(), here.cigar.tolist())
    assert n_pairs > 2500 and n_overlap > 500                  # the clipping of overlapping mates is exercised
    assert (flagged.flag & 0x8).sum() > 50 and (flagged.next_ref == 1).sum() > 50      # orphans, and mates on the other reference
    return paths[0], paths[1], chrom, ov, gene_df, exon_df


@pytest.mark.parametrize('mode', ['host', 'device'])
def test_flag_rule_equals_the_name_rule_on_the_twin(mode, twins, tmp_path):
    flagged, twin, chrom, ov, gene_df, exon_df = twins
    kw = dict(inflate=mode, frame=mode, window_bytes=20000, chroms=[chrom])
    proc, got = _run(flagged, chrom, ov, gene_df, exon_df, tmp_path / 'flag', pairing='flag', **kw)
    assert proc.paired and proc.pairing_rule == 'flag' and proc.timing['pair_device_ms'] > 0
    assert len(list(proc._batches(chrom))) > 2                 # mates lie in different windows
    assert proc.dropped['not_candidate'] > 100 and proc.dropped['flags'] == proc.dropped['mapq'] == 0
    name_proc, want = _run(twin, chrom, ov, gene_df, exon_df, tmp_path / 'name', pair='device', **kw)
    assert name_proc.paired and name_proc.pairing_rule == 'name'
    _same(got, want)
    assert int(got[2].iloc[:, 1].sum()) > 500
    plain, each = _run(flagged, chrom, ov, gene_df, exon_df, tmp_path / 'default', **kw)
    assert not plain.paired and int(each[2].iloc[:, 1].sum()) > int(got[2].iloc[:, 1].sum())      # the default counts mates as reads


def test_flag_rule_run_to_run(twins, tmp_path):
    flagged, _, chrom, ov, gene_df, exon_df = twins
    kw = dict(pairing='flag', inflate='device', frame='device', chroms=[chrom], exclude_flags=0x900, min_mapq=1)
    _, a = _run(flagged, chrom, ov, gene_df, exon_df, tmp_path / 'a', **kw)
    _, b = _run(flagged, chrom, ov, gene_df, exon_df, tmp_path / 'b', **kw)
    _same(a, b)
    for name in sorted(os.listdir(str(tmp_path / 'a'))):
        for f in sorted(os.listdir(str(tmp_path / 'a' / name))):
            if f.endswith('.npz'):
                continue                                       # a zip archive: it holds the time it was written
            with open(str(tmp_path / 'a' / name / f), 'rb') as fa, open(str(tmp_path / 'b' / name / f), 'rb') as fb:
                assert fa.read() == fb.read(), f


# --- hand-made compositions on the two-gene layout --------------------------------------------------------------------------

def _counts(tmp_path, name, records, paired=None, refs=None, **kw):
    """Gene counts, CSR row, processor and the chromosome's reads frame of the records on the two-gene layout (genes X, Y)."""
    chrom_len, gene_df, exon_df, ov = _two_gene_case()
    p = str(tmp_path / (name + '.bam'))
    fc.write_bam(p, refs or [('c', chrom_len)], fc.rows(records))
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / (name + '_out')), verbose=False, chroms=['c'], **kw)
    if paired is not None:
        proc.paired = paired                                   # the rule under test, whatever the decision says
    os.makedirs(proc.save_dir, exist_ok=True)
    proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, 'c')
    csr, _, cnt = _files(proc, 'c')
    return dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int))), csr, proc


PAIR_X = [('ok', 110, '20M', F, 250), ('ok', 250, '20M', L, 110)]      # one good pair on gene X in every file


def test_two_first_mates_and_no_last_count_nothing(tmp_path):
    counts, _, proc = _counts(tmp_path, 'ff', PAIR_X + [('d', 1010, '20M', F, 1100), ('d', 1010, '20M', F, 1100)], pairing='flag')
    assert proc.paired and counts == {'X': 1, 'Y': 0}


def test_a_key_with_three_rows_counts_nothing(tmp_path):
    recs = PAIR_X + [('t', 1010, '20M', F, 1100), ('t', 1100, '20M', L, 1010), ('t', 1100, '20M', L, 1010)]
    counts, _, _ = _counts(tmp_path, 'three', recs, pairing='flag')
    assert counts == {'X': 1, 'Y': 0}


@pytest.mark.parametrize('what,first,last', [
    ('mate_unmapped', F | 0x8, L | 0x8),
    ('unmapped', F | 0x4, L),
    ('not_paired', 0x40, 0x80),
    ('both_bits', 0x1 | 0x40 | 0x80, L),
    ('neither_bit', 0x1, L),
])
def test_records_that_are_no_candidates_are_not_stored(what, first, last, tmp_path):
    recs = PAIR_X + [('n', 1010, '20M', first, 1100), ('n', 1100, '20M', last, 1010)]
    counts, _, proc = _counts(tmp_path, what, recs, pairing='flag')
    n_bad = 2 if what in ('mate_unmapped', 'not_paired') else 1
    assert counts == {'X': 1, 'Y': 0} and proc.dropped == {'flags': 0, 'mapq': 0, 'not_candidate': n_bad}
    frame = proc.load_chromosome_reads('c')
    assert frame.columns.tolist() == ['qname', 'pos', 'cigar', 'flag', 'mapq', 'pnext', 'qname_unpaired']
    assert len(frame) == 4 - n_bad and frame.pos.tolist() == sorted(frame.pos.tolist()) and (frame.qname == frame.qname_unpaired).all()
    assert frame.flag.tolist()[:2] == [F, L] and frame.pnext.tolist()[:2] == [250, 110] and frame.mapq.tolist()[:2] == [60, 60]


def test_a_mate_on_another_reference_is_not_stored(tmp_path):
    recs = PAIR_X + [('n', 1010, '20M', F, 1100, 1), ('n', 1100, '20M', L, 1010, 1), ('m', 1020, '20M', F, 5, -1)]
    counts, _, proc = _counts(tmp_path, 'elsewhere', recs, pairing='flag', refs=[('c', 2000), ('d', 2000)])
    assert counts == {'X': 1, 'Y': 0} and proc.dropped['not_candidate'] == 3


def test_one_template_at_two_loci_counts_two_pairs(tmp_path):
    recs = [('m', 110, '20M', F, 250), ('m', 250, '20M', L, 110), ('m', 1010, '20M', F | 0x100, 1100), ('m', 1100, '20M', L | 0x100, 1010)]
    counts, _, _ = _counts(tmp_path, 'loci', recs, pairing='flag', unique_alignment=False)
    assert counts == {'X': 1, 'Y': 1}
    # the name rule on the same file: four rows share one name (and one qname_unpaired, the empty one)
    counts, _, proc = _counts(tmp_path, 'loci_name', recs, paired=True, unique_alignment=False, pair='device')
    assert proc.pairing_rule == 'name' and counts == {'X': 0, 'Y': 0}


def test_mate_inside_its_mate_follows_file_order(tmp_path):
    """
    The expectation of test_gpu_pair.test_mate_inside_its_mate_follows_file_order: A = [150, 179] comes first in the file and is
    mate 1 of the clipping although it is the template's last segment (0x80); B = [155, 164] is clipped to 149.
    """
    counts, csr, _ = _counts(tmp_path, 'inside', [('m', 150, '30M', L, 155), ('m', 155, '10M', F, 150)], pairing='flag')
    expect = np.zeros(2000, dtype=np.int64)
    expect[149:180] = 1
    assert np.array_equal(csr.toarray().ravel(), expect) and counts == {'X': 1, 'Y': 0}


def test_the_position_prefilter_comes_before_the_count_of_a_key(tmp_path):
    """Of a key's three rows one ends past the last gene's end + 1 (the pre-filter drops it): the two that are left are a pair."""
    recs = [('k', 1010, '20M', F, 1100), ('k', 1100, '20M', L, 1010), ('k', 1100, '300M', L, 1010)]
    counts, _, _ = _counts(tmp_path, 'prefilter', recs, pairing='flag')
    assert counts == {'X': 0, 'Y': 1}


# --- the read filters ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def noisy():
    """Single-end reads on the golden layout with MAPQ 9, 10, 11 and 255 and the FLAG bits the filters are asked about."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(17, 1500, False)
    rng = np.random.default_rng(6)
    n = len(src)
    flag = rng.choice([0, 0x10, 0x2, 0x2 | 0x10, 0x4, 0x100, 0x400, 0x800, 0x100 | 0x400, 0x200], n, p=[.3, .2, .1, .1, .06, .06, .06, .06, .03, .03])
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values, 'flag': flag, 'next_ref': -1,
                       'next_pos': -1, 'mapq': rng.choice([9, 10, 11, 255], n)})
    return chrom, chrom_len, gene_df, exon_df, ov, df


FILTERS = [dict(min_mapq=10), dict(exclude_flags=0x4), dict(exclude_flags=0x100), dict(exclude_flags=0x400), dict(exclude_flags=0x800),
           dict(exclude_flags=0xF04), dict(require_flags=0x2), dict(exclude_flags=0x904, require_flags=0x2, min_mapq=11)]


@pytest.mark.parametrize('opt', FILTERS, ids=['-'.join('{0}{1}'.format(k[:3], v) for k, v in sorted(o.items())) for o in FILTERS])
@pytest.mark.parametrize('mode', ['host', 'device'])
def test_filters_equal_the_file_without_the_records(opt, mode, noisy, tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, df = noisy
    by_flags = ((df.flag & opt.get('exclude_flags', 0)) != 0) | ((df.flag & opt.get('require_flags', 0)) != opt.get('require_flags', 0))
    by_mapq = ~by_flags & (df.mapq < opt.get('min_mapq', 0))
    assert 0 < int(by_flags.sum()) + int(by_mapq.sum()) < len(df)
    (tmp_path / 'full').mkdir()
    (tmp_path / 'less').mkdir()
    full, less = str(tmp_path / 'full' / 's.bam'), str(tmp_path / 'less' / 's.bam')     # one sample name: it heads a column of the counts
    fc.write_bam(full, [(chrom, chrom_len)], df, straddle=True)
    fc.write_bam(less, [(chrom, chrom_len)], df[~by_flags & ~by_mapq], straddle=True)
    kw = dict(inflate=mode, frame=mode, window_bytes=30000)
    proc, got = _run(full, chrom, ov, gene_df, exon_df, tmp_path / 'got', **dict(kw, **opt))
    _, want = _run(less, chrom, ov, gene_df, exon_df, tmp_path / 'want', **kw)
    _same(got, want)
    assert proc.dropped == {'flags': int(by_flags.sum()), 'mapq': int(by_mapq.sum()), 'not_candidate': 0}
    assert int(got[2].iloc[:, 1].sum()) > 100
    pd.testing.assert_frame_equal(proc.load_chromosome_reads(chrom), bam.NativeBamReadsProcessor(
        less, less + '.bai', output_dir=str(tmp_path / 'o'), verbose=False).load_chromosome_reads(chrom))


def test_filters_on_a_file_paired_by_name(tmp_path):
    """A .1 / .2 file: a mate the filter drops leaves its partner alone, which then counts nothing."""
    recs = []
    for i in range(40):
        recs += [('p{0}.1'.format(i), 110 + 2 * i, '20M', 0, 250 + i, 0, 5 if i % 4 == 0 else 30),
                 ('p{0}.2'.format(i), 250 + i, '25M', 0x400 if i % 4 == 1 else 0, 110 + 2 * i, 0, 30)]
    counts, _, proc = _counts(tmp_path, 'named', recs, min_mapq=10, exclude_flags=0x400)
    assert proc.paired and proc.pairing_rule == 'name' and counts == {'X': 20, 'Y': 0}
    assert proc.dropped == {'flags': 10, 'mapq': 10, 'not_candidate': 0}
    counts, _, _ = _counts(tmp_path, 'named_all', recs)
    assert counts == {'X': 40, 'Y': 0}


def test_placed_unmapped_mates_need_exclude_flags_4(tmp_path):
    """Unmapped mates kept "within" a sorted file: FLAG 0x4, placed at the mate's position, no CIGAR."""
    recs = []
    for i in range(30):
        recs += [('g{0}'.format(i), 110 + 2 * i, '20M', F, 250 + i), ('g{0}'.format(i), 250 + i, '25M', L, 110 + 2 * i)]
    recs += [('u{0}'.format(i), 120 + i, '20M', F | 0x8, 120 + i) for i in range(5)]
    recs += [('u{0}'.format(i), 120 + i, None, L | 0x4, 120 + i) for i in range(5)]
    for kw in (dict(), dict(min_mapq=1), dict(require_flags=0x1)):
        with pytest.raises(ValueError, match='read u0 has no CIGAR string'):
            _counts(tmp_path, 'raises' + '_'.join(kw), recs, **kw)
    # the FLAG rule takes no record with 0x4 for a candidate, so it never sees the missing CIGAR
    counts, _, proc = _counts(tmp_path, 'flag_only', recs, pairing='flag')
    assert counts == {'X': 30, 'Y': 0} and proc.dropped == {'flags': 0, 'mapq': 0, 'not_candidate': 10}
    counts, _, proc = _counts(tmp_path, 'clean', recs, pairing='flag', exclude_flags=4)
    assert counts == {'X': 30, 'Y': 0} and proc.dropped == {'flags': 5, 'mapq': 0, 'not_candidate': 5}
    counts, _, proc = _counts(tmp_path, 'clean_se', recs, exclude_flags=4)
    assert not proc.paired and counts == {'X': 65, 'Y': 0} and proc.dropped == {'flags': 5, 'mapq': 0, 'not_candidate': 0}


def test_a_filtered_record_raises_none_of_the_errors_of_a_kept_row():
    """NH of a non-integer type, an op code above 8: errors of kept rows only."""
    df = fc.rows([('a', 110, '20M', 0, -1, -1), ('bad_nh', 120, '20M', 0x400, -1, -1), ('bad_op', 130, '20M', 0x400, -1, -1)])
    df = df.assign(nh=[1, 2, 1], nh_type=['C', 'Z', 'C'])
    data, offs = fc.encode(df)
    data = bytearray(data)
    o = int(offs[2])
    at = o + 36 + data[o + 12]
    data[at] = (data[at] & 0xf0) | 9                             # op code 9
    for kw, text in ((dict(), 'NH tag of a non-integer type'), (dict(exclude_flags=0x400), None)):
        rows = bam.DeviceRows(0, True, False, **kw)
        try:
            if text:
                with pytest.raises(ValueError, match=text):
                    rows.append(bytes(data), offs)
            else:
                rows.append(bytes(data), offs)
                assert rows.info()[0] == 1 and rows.dropped() == (2, 0, 0)
        finally:
            rows.close()


def test_a_malformed_record_is_refused_whatever_the_filters_say():
    df = fc.rows([('a', 110, '20M', 0, -1, -1), ('broken', 120, '20M', 0x400, -1, -1, 0)])
    data, offs = fc.encode(df)
    data = bytearray(data)
    data[fc.aux_offset(data, int(offs[1])) + 2] = ord('!')      # an aux field of an unknown type
    for kw in (dict(), dict(exclude_flags=0x400), dict(min_mapq=10), dict(require_flags=0x2), dict(exclude_flags=0xffff, min_mapq=255)):
        rows = bam.DeviceRows(0, True, False, **kw)
        try:
            with pytest.raises(ValueError, match=r'malformed BAM record \(read broken\)'):
                rows.append(bytes(data), offs)
        finally:
            rows.close()


# --- a standard file under the default, and under 'auto' ----------------------------------------------------------------------

def _standard(n=40):
    recs = []
    for i in range(n):
        recs += [('g{0}'.format(i), 110 + 2 * i, '20M', F | 0x2, 250 + i), ('g{0}'.format(i), 250 + i, '25M', L | 0x2, 110 + 2 * i)]
    return recs


def test_the_default_takes_a_standard_paired_file_for_single_end(tmp_path):
    """What the reference's rule does with an aligner's names: each mate is a read.  The behaviour before this option too."""
    chrom_len, gene_df, exon_df, ov = _two_gene_case()
    p = str(tmp_path / 's.bam')
    fc.write_bam(p, [('c', chrom_len)], fc.rows(_standard()))
    proc, (_, _, cnt) = _run(p, 'c', ov, gene_df, exon_df, tmp_path / 'out')
    assert proc.paired is False
    assert dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int))) == {'X': 80, 'Y': 0}


def test_auto_pairs_a_standard_file_and_leaves_a_named_one_to_the_name_rule(tmp_path):
    counts, _, proc = _counts(tmp_path, 'auto', _standard(), pairing='auto')
    assert (proc.paired, proc.pairing_rule) == (True, 'flag') and counts == {'X': 40, 'Y': 0}
    named = [(q + ('.1' if f & 0x40 else '.2'), pos, cig, f, pnext) for q, pos, cig, f, pnext in _standard()]
    named += [('g0.1', 300, '20M', F, 250)]                    # a third g0: the name rule drops the name, the FLAG rule would not
    counts, _, proc = _counts(tmp_path, 'auto_named', named, pairing='auto')
    assert (proc.paired, proc.pairing_rule) == (True, 'name') and counts == {'X': 39, 'Y': 0}


# --- the command ----------------------------------------------------------------------------------------------------------------

def _sample(k):
    """(flag-style rows with what the filters are to remove, their renamed and pre-filtered twin) of sample k: two chromosomes."""
    import _gtf_fixtures as gf
    parts_f, parts_t = [], []
    for tid, (layout, n, skip) in enumerate(((rf.golden_layout(), 300, ('I',)), (rf.quiet_layout(), 100, ('R',)))):
        flagged, twin = fc.flag_style(rf.synth_pairs(70 + 10 * tid + k, layout, n, skip=skip), ref=tid, seed=k, elsewhere=0.0)
        rng = np.random.default_rng(90 + k + tid)
        low = rng.random(len(flagged)) < 0.05                   # a mate below the MAPQ bound: its partner is left alone
        # `place` orders the SAM lines: the twin keeps the relative order of its records, so that mates at one position come
        # in the same order in both sorted files (mate 1 of the clipping is the first in the file)
        place = rng.random(len(flagged))
        flagged, twin = flagged.assign(mapq=np.where(low, 5, 30), place=place), twin.assign(mapq=np.where(low, 5, 30), place=place)
        extra = flagged.sample(25, random_state=k).assign(flag=lambda d: d.flag | rng.choice([0x100, 0x800, 0x900], len(d)),
                                                          place=lambda d: rng.random(len(d)))
        lost = flagged.sample(10, random_state=k + 1).assign(flag=lambda d: (d.flag ^ 0xC0) | 0x4, cigar=None,
                                                             place=lambda d: rng.random(len(d)))     # placed unmapped mates
        parts_f += [flagged, extra, lost]
        parts_t.append(twin[~low])
    assert gf.PIPELINE_REFS[0][1] == 6000 and gf.PIPELINE_REFS[1][1] == 2000
    return pd.concat(parts_f, ignore_index=True), pd.concat(parts_t, ignore_index=True)


def _write_sam(path, refs, reads):
    reads = reads.sort_values('place', kind='stable')
    assert not reads.pos.is_monotonic_increasing
    with open(path, 'w') as f:
        f.write(fc.sam_header(refs) + fc.sam_text(reads, refs))


def test_command_with_pair_by_flag_equals_the_command_on_the_twins(tmp_path):
    import _gtf_fixtures as gf
    from test_gpu_pipeline import GTF, RESULT_FILES
    refs = gf.PIPELINE_REFS
    outs = []
    for which, flags in ((0, ['--pair-by', 'flag', '--exclude-flags', '0x904', '--min-mapq', '10']), (1, ['--device-pair'])):
        d = tmp_path / ('in{0}'.format(which))
        d.mkdir()
        paths = []
        for k, s in enumerate(gf.PIPELINE_SAMPLES):
            p = str(d / (s + '.sam'))
            _write_sam(p, refs, _sample(k)[which])
            paths.append(p)
        out = str(tmp_path / ('out{0}'.format(which)))
        cmd = [sys.executable, '-m', 'degnorm_amd', '--device-inflate', '--device-frame', '--sam-files'] + paths + flags + \
              ['-g', GTF, '-o', out, '--iter', '2', '--nmf-iter', '20', '--minimax-coverage', '1']     # gene I has no reads
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
        assert r.returncode == 0, r.stdout[-4000:]
        assert r.stdout.count('sample contains paired reads') == 3, r.stdout[-4000:]
        if which == 0:
            assert 'dropped by flags' in r.stdout and 'not a mate candidate' in r.stdout
        outs.append(out)
    a, b = outs
    counts = pd.read_csv(os.path.join(a, 'read_counts.csv'))
    assert counts[gf.PIPELINE_SAMPLES].values.sum() > 200
    names = ['read_counts.csv', 'gene_exon_metadata.csv'] + RESULT_FILES + \
            [os.path.join(c, 'coverage_matrices_{0}.pkl'.format(c)) for c in ('chr1', 'chr2')]
    for name in names:
        with open(os.path.join(a, name), 'rb') as fa, open(os.path.join(b, name), 'rb') as fb:
            assert fa.read() == fb.read(), name
