"""
Strand-specific counting without a GPU (the rule: include/degnorm_amd.h, "Strand-specific counting"):

  sense rule       the library's host build of dn::row_sense (csrc/dn_bam_record.hpp, through dn_read_sense_host) against
                   the plain restatement of tests/_strand_cases.py, for every combination of FLAG 0x1, 0x10, 0x40, 0x80, a
                   name ending in .1 / .2 / neither, the three kinds of store and the two protocols
  hand-made case   the counts written out in _strand_cases.HAND_COUNTS are what the restatement of tests/_reads_oracle.py
                   gives on the per-strand annotation and the rows of that sense (and, unstranded, on all of it)
  option checking  every bad `stranded` value is a ValueError before a file is opened; the pysam-backed reader refuses the
                   option; a strand selector that is not '+' or '-', a sense column of another length or alphabet
"""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_oracle as ro                                      # noqa: E402
import _strand_cases as sc                                      # noqa: E402
from degnorm_amd import bam as db                              # noqa: E402
from degnorm_amd import reads as dr                            # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure   # noqa: E402

BAD_STRANDED = ('yes', 'Forward', 'REVERSE', '', 'fr', None, 0, 1, 2, True, False, b'forward', ('forward',), ['no'])


# --- the sense rule -------------------------------------------------------------------------------------------------------

def _combinations():
    bits = (0x1, 0x10, 0x40, 0x80)
    flags = [sum(b for b, on in zip(bits, mask) if on) for mask in itertools.product((0, 1), repeat=4)]
    assert len(flags) == 16 and len(set(flags)) == 16
    return [(f, n) for f in flags for n in ('g7.1', 'g7.2', 'read7', '2', '')]


@pytest.mark.parametrize('protocol', sc.PROTOCOLS)
@pytest.mark.parametrize('store', sc.STORE_KINDS)
def test_host_build_of_the_sense_rule_equals_the_restatement(store, protocol):
    cases = _combinations()
    flags, names = [f | 0x400 if k % 3 == 0 else f for k, (f, _) in enumerate(cases)], [n for _, n in cases]   # a bit the rule does not read
    got = dr.row_sense(flags, names, store == 'name', protocol)
    want = [sc.sense_rule(f, n, store, protocol) for f, n in zip(flags, names)]
    assert got == want
    assert set(got) == {'+', '-'}
    # the other protocol is the flip, row for row
    other = dr.row_sense(flags, names, store == 'name', 'reverse' if protocol == 'forward' else 'forward')
    assert all(a != b for a, b in zip(got, other))


def test_the_rule_by_hand():
    # single read / first mate: the strand it aligned to; last mate: the other one; the name rule reads the name's last byte
    assert dr.row_sense([0, 16, 0x41, 0x51, 0x81, 0x91, 0x80, 0x90], ['r'] * 8, False, 'forward') == list('+-+--+' + '+-')
    assert dr.row_sense([0, 16, 0, 16], ['g.1', 'g.1', 'g.2', 'g.2'], True, 'forward') == list('+--+')
    assert dr.row_sense([0, 16, 0, 16], ['g.1', 'g.1', 'g.2', 'g.2'], False, 'forward') == list('+-+-')
    assert dr.row_sense([0x81, 0x81], ['g.2', 'g.1'], True, 'reverse') == list('++')      # both marks make one flip, not two
    assert dr.row_sense([], [], True, 'forward') == []


def test_row_sense_refuses_what_has_no_sense():
    with pytest.raises(ValueError, match="'forward' or 'reverse' only"):
        dr.row_sense([0], ['a'], False, 'no')
    with pytest.raises(ValueError, match='one name per FLAG'):
        dr.row_sense([0, 16], ['a'], False, 'forward')


# --- the hand-made case -------------------------------------------------------------------------------------------------

def _hand_senses(reads, protocol):
    return np.array([sc.sense_rule(int(f), q, 'single', protocol) for f, q in zip(reads.flag, reads.qname)], dtype=object)


def test_hand_case_shape():
    reads, chrom_len, gene_df, exon_df, strand_of = sc.hand_case()
    both = get_gene_overlap_structure(gene_df)
    assert both == {'overlap_genes': [['P', 'M'], ['A', 'B']], 'isolated_genes': ['IP', 'IM']}
    parts = sc.split_tables(gene_df, exon_df, strand_of)
    assert parts['+'][0] == {'overlap_genes': [['A', 'B']], 'isolated_genes': ['P', 'IP']}
    assert parts['-'][0] == {'overlap_genes': [], 'isolated_genes': ['M', 'IM']}


def test_hand_written_counts_are_the_restatement_s():
    reads, chrom_len, gene_df, exon_df, strand_of = sc.hand_case()
    plain = ro.restate(reads, chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df, False)
    assert plain[2] == sc.HAND_COUNTS['no'] and plain[3]['caught_2plus'] == 3          # r0, r1 and r7
    parts = sc.split_tables(gene_df, exon_df, strand_of)
    for protocol in sc.PROTOCOLS:
        sense = _hand_senses(reads, protocol)
        counts = {}
        for s in sc.STRANDS:
            counts.update(sc.expected(reads, sense, chrom_len, parts, s, False)[2])
        assert counts == sc.HAND_COUNTS[protocol], protocol
    # a read in the shared exon is dropped unstranded and counted once on its strand
    sense = _hand_senses(reads, 'forward')
    assert sense[0] == '+' and sense[1] == '-'
    first_two = reads.iloc[:2]
    assert sum(ro.restate(first_two, chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df, False)[2].values()) == 0
    assert sc.expected(first_two, sense[:2], chrom_len, parts, '+', False)[2]['P'] == 1
    assert sc.expected(first_two, sense[:2], chrom_len, parts, '-', False)[2]['M'] == 1


def test_seeded_cases_are_seeded_and_have_what_they_are_for():
    a = sc.stranded_case(13, True, None)
    b = sc.stranded_case(13, True, None)
    assert a[0].equals(b[0]) and (a[1] == b[1]).all() and a[5] == b[5]
    reads, sense, chrom_len, gene_df, exon_df, strand_of = a
    assert 2700 < len(reads) < 3300 and set(sense) == {'+', '-'} and set(strand_of.values()) == {'+', '-'}
    assert len(sc.disagreeing_pairs(reads, sense)) >= 20
    one = sc.stranded_case(13, False, 64, one_strand=True)
    assert set(one[5].values()) == {'+'} and list(sc.split_tables(one[3], one[4], one[5])) == ['+']


# --- option checking ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bad', BAD_STRANDED, ids=repr)
def test_a_bad_stranded_value_is_refused_before_a_file_is_opened(bad, tmp_path):
    missing = str(tmp_path / 'missing.bam')
    with pytest.raises(ValueError, match='stranded must be'):
        dr.check_stranded(bad)
    with pytest.raises(ValueError, match='stranded must be'):
        db.NativeBamReadsProcessor(missing, missing + '.bai', stranded=bad)
    with pytest.raises(ValueError, match='stranded must be'):
        dr.BamReadsProcessor(missing, missing + '.bai', stranded=bad)
    with pytest.raises(ValueError, match='stranded must be'):
        db.DeviceRows(0, True, False, stranded=bad)
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize('mode', sc.PROTOCOLS)
def test_the_pysam_reader_does_not_count_by_strand(mode, tmp_path):
    missing = str(tmp_path / 'missing.bam')
    with pytest.raises(ValueError, match='needs bam.NativeBamReadsProcessor'):
        dr.BamReadsProcessor(missing, missing + '.bai', stranded=mode)


def test_good_values_pass():
    assert [dr.check_stranded(m) for m in ('no', 'forward', 'reverse')] == ['no', 'forward', 'reverse']
    assert dr.STRANDED == ('no', 'forward', 'reverse')


def test_sense_and_strand_are_checked_before_the_device_is_touched():
    reads, chrom_len, gene_df, exon_df, strand_of = sc.hand_case()
    ov, g, e = sc.split_tables(gene_df, exon_df, strand_of)['+']
    sense = _hand_senses(reads, 'forward')
    call = dr.chromosome_coverage_read_counts_df
    with pytest.raises(ValueError, match='sense and strand go together'):
        call(reads, chrom_len, ov, g, e, False, sense=sense)
    with pytest.raises(ValueError, match='sense and strand go together'):
        call(reads, chrom_len, ov, g, e, False, strand='+')
    for bad in ('.', '?', 'plus', '', 43, b'+'):
        with pytest.raises(ValueError, match="strand must be '\\+' or '-'"):
            dr.check_strand(bad)
    with pytest.raises(ValueError, match="sense must hold '\\+' or '-' for every row"):
        dr.pack_sense(sense[:-1], len(reads))
    with pytest.raises(ValueError, match="sense must hold '\\+' or '-' for every row"):
        dr.pack_sense(['+'] * (len(reads) - 1) + ['.'], len(reads))
    assert dr.pack_sense(['+', '-'], 2).tolist() == [43, 45] and dr.pack_sense(np.array([43, 45], np.uint8), 2).tolist() == [43, 45]


# --- the strand column of the GFF3 scan, host build -----------------------------------------------------------------------

import logging                                                  # noqa: E402

import pandas as pd                                             # noqa: E402

import _gff3_fixtures as g3                                     # noqa: E402
from degnorm_amd import loaders                                 # noqa: E402
from degnorm_amd.gene_processing import GeneAnnotationProcessor  # noqa: E402

BAD_FIELDS = (b'x', b'', b'++')
STRAND_TEXT = 'is an exon record whose strand (column 7) is not one of + - . ?'


@pytest.fixture(scope='module')
def dialect_texts(tmp_path_factory):
    d = tmp_path_factory.mktemp('strand_gff3')
    out = {}
    for dialect in g3.DIALECTS:
        p = str(d / (dialect + '.gff3'))
        g3.write_gff3(p, 3, 12, dialect)
        with open(p, 'rb') as f:
            out[dialect] = f.read()
    return out


@pytest.mark.parametrize('dialect', g3.DIALECTS)
def test_host_strand_column_is_field_seven_of_the_exon_line(dialect, dialect_texts):
    data = dialect_texts[dialect]
    n, cols, err = loaders.gff3_scan(data, strand=True)
    n0, cols0, err0 = loaders.gff3_scan(data)
    assert err is None and err0 is None and n == n0 and 'strand' not in cols0
    for k in cols0:
        assert cols[k].tobytes() == cols0[k].tobytes(), k
    want = sc.field7(data, fasta=True)
    assert cols['strand'].tobytes() == b''.join(want) and set(want) == {b'+', b'-'}      # the fixture's genes alternate strands


def test_host_strand_column_on_hand_written_lines():
    ln = g3._ln
    gene = ln('c1', 'gene', 1, 900, 'ID=g1;Name=G')
    text = b'\n'.join([gene] + [ln('c1', 'exon', 10 * k + 1, 10 * k + 9, 'Parent=g1').replace(b'\t.\t+\t.\t', b'\t.\t' + s.encode() + b'\t.\t')
                                 for k, s in enumerate('+-.?+')]) + b'\n'
    assert sc.field7(text, True) == [b'+', b'-', b'.', b'?', b'+']
    n, cols, err = loaders.gff3_scan(text, strand=True)
    assert err is None and cols['strand'].tobytes() == b'+-.?+'
    # behind ##FASTA nothing is read, whatever its seventh field says
    tail = text + b'##FASTA\n' + ln('c1', 'exon', 1, 9, 'Parent=g1').replace(b'\t+\t', b'\tx\t')
    n, cols, err = loaders.gff3_scan(tail, strand=True)
    assert err is None and cols['strand'].tobytes() == b'+-.?+'


@pytest.mark.parametrize('bad', BAD_FIELDS)
def test_a_bad_strand_field_is_a_malformed_line_only_when_the_strand_is_asked_for(bad, dialect_texts):
    data = dialect_texts['ensembl']
    at = sc.exon_lines(data)
    for line in (at[0], at[5], at[-1]):
        text = sc.with_field7(data, line, bad)
        n, cols, err = loaders.gff3_scan(text, strand=True)
        assert err == (line, 6) and all(len(v) == 0 for v in cols.values())
        with pytest.raises(ValueError) as e:
            sc.field7(text, True)
        assert e.value.args[0] == (line, 'strand')
        n0, cols0, err0 = loaders.gff3_scan(text)                # not asked for: as today, nothing about field seven is checked
        clean = loaders.gff3_scan(data)
        assert err0 is None and n0 == clean[0] and all(cols0[k].shape == clean[1][k].shape for k in cols0)
        assert cols0['start'].tobytes() == clean[1]['start'].tobytes() and cols0['line'].tobytes() == clean[1]['line'].tobytes()
    # the first faulty line wins, whatever its fault: a line with too few fields above the bad strand, and below it
    lines = data.split(b'\n')
    above = b'\n'.join(lines[:at[2] - 1] + [b'c1\tx\texon\t1'] + lines[at[2] - 1:])
    assert loaders.gff3_scan(sc.with_field7(above, at[5] + 1, bad), strand=True)[2] == (at[2], 1)
    below = b'\n'.join(lines[:at[8] - 1] + [b'c1\tx\texon\t1'] + lines[at[8] - 1:])
    assert loaders.gff3_scan(sc.with_field7(below, at[5], bad), strand=True)[2] == (at[5], 6)
    assert loaders._GFF3_KINDS[6] == STRAND_TEXT and loaders._KINDS[4] == STRAND_TEXT


# --- the gene rule ----------------------------------------------------------------------------------------------------------

def _exons(rows):
    return pd.DataFrame(rows, columns=['chr', 'start', 'end', 'gene', 'strand'])


def test_gene_rule_keeps_genes_of_one_strand_and_names_the_others(caplog):
    rows = [('c1', 1, 10, 'plus', '+'), ('c1', 21, 30, 'plus', '+'),
            ('c1', 41, 50, 'minus', '-'),
            ('c1', 61, 70, 'mixed', '+'), ('c1', 81, 90, 'mixed', '-'),
            ('c1', 101, 110, 'dot', '.'), ('c1', 121, 130, 'dot', '.'),
            ('c1', 141, 150, 'partly', '+'), ('c1', 161, 170, 'partly', '.'),
            ('c1', 181, 190, 'what', '?')]
    proc = GeneAnnotationProcessor('unused.gtf', verbose=False, strand=True)
    with caplog.at_level(logging.WARNING):
        out = proc.process(_exons(rows))
    assert proc.unstranded_genes == ['mixed', 'dot', 'partly', 'what']
    assert out.gene.tolist() == ['plus', 'plus', 'minus'] and out.strand.tolist() == ['+', '+', '-']
    assert list(out.columns) == ['chr', 'start', 'end', 'gene', 'strand', 'gene_start', 'gene_end']
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and warned[0].startswith('4 genes without a single strand') and warned[0].endswith('mixed, dot, partly, what')
    # all agree: nothing is left out and nothing is said
    caplog.clear()
    proc = GeneAnnotationProcessor('unused.gtf', verbose=False, strand=True)
    with caplog.at_level(logging.WARNING):
        out = proc.process(_exons(rows[:3]))
    assert proc.unstranded_genes == [] and len(out) == 3 and not caplog.records
    # more than ten: the count and ten names
    many = [('c1', 10 * k + 1, 10 * k + 5, 'u{0:02d}'.format(k), '.') for k in range(13)] + rows[:1]
    proc = GeneAnnotationProcessor('unused.gtf', verbose=False, strand=True)
    with caplog.at_level(logging.WARNING):
        out = proc.process(_exons(many))
    assert len(proc.unstranded_genes) == 13 and out.gene.tolist() == ['plus']
    text = caplog.records[-1].getMessage()
    assert text.startswith('13 genes') and 'u09, ...' in text and 'u10' not in text
    # without the argument the table is today's, column for column
    plain = GeneAnnotationProcessor('unused.gtf', verbose=False).process(_exons(rows).drop(columns='strand'))
    assert list(plain.columns) == ['chr', 'start', 'end', 'gene', 'gene_start', 'gene_end'] and plain.gene.nunique() == 6
