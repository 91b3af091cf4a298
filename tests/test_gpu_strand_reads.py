"""
GPU tests of strand-specific counting at the kernel (the stranded instances of k_prefilter, csrc/dn_reads.hip), through
reads.chromosome_coverage_read_counts_df(..., sense=, strand=).  The rule and its guarantee are in include/degnorm_amd.h,
"Strand-specific counting": a stranded call on one strand's annotation gives what the unstranded code gives on that
annotation and the rows of that sense.  Every comparison is exact.

  hand-made case   an opposite-strand pair of genes that share an exon, one isolated gene per strand, a two-gene overlap
                   group on '+'; ten reads with their counts written out (unstranded, forward, reverse)
  restatement      tests/_reads_oracle.restate on the rows pre-filtered by sense and the per-strand annotation: single-end
                   and paired, 0, 1, 63, 64, 65, 255, 256, 257 and about 3 000 rows (the pre-filter's block size is 256),
                   senses all '+', all '-' and mixed, a strand without genes, pairs whose mates disagree
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_oracle as ro                                      # noqa: E402
import _strand_cases as sc                                      # noqa: E402
from degnorm_amd import reads as dr                            # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure   # noqa: E402

pytestmark = pytest.mark.gpu

ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, None)           # None: the whole case, about 3 000 rows
SEED = 13


def _stranded_counts(reads, sense, chrom_len, parts, paired=False):
    out = {}
    for s, (ov, g, e) in parts.items():
        out[s] = dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, g, e, paired, sense=sense, strand=s)
    return out


# --- the hand-made case -------------------------------------------------------------------------------------------------

def test_hand_made_case_counts_by_strand():
    reads, chrom_len, gene_df, exon_df, strand_of = sc.hand_case()
    parts = sc.split_tables(gene_df, exon_df, strand_of)
    plain = dr.chromosome_coverage_read_counts_df(reads, chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df, False)
    assert plain[2] == sc.HAND_COUNTS['no']
    got = {}
    for protocol in sc.PROTOCOLS:
        sense = dr.row_sense(reads.flag.values, reads.qname.tolist(), False, protocol)
        assert sense == [sc.sense_rule(int(f), q, 'single', protocol) for f, q in zip(reads.flag, reads.qname)]
        out = _stranded_counts(reads, sense, chrom_len, parts)
        counts = {}
        for s in sc.STRANDS:
            assert list(out[s][2]) == parts[s][1].gene.tolist()
            counts.update(out[s][2])
            ro.assert_same(out[s], sc.expected(reads, np.array(sense, dtype=object), chrom_len, parts, s, False), protocol + s)
        assert counts == sc.HAND_COUNTS[protocol], protocol
        got[protocol] = out
    # the two reads in the shared exon: dropped unstranded, counted once each on their strands
    two = reads.iloc[:2]
    assert sum(dr.chromosome_coverage_read_counts_df(two, chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df, False)[2].values()) == 0
    out = _stranded_counts(two, ['+', '-'], chrom_len, parts)
    assert out['+'][2] == {'P': 1, 'IP': 0, 'A': 0, 'B': 0} and out['-'][2] == {'M': 1, 'IM': 0}
    # P is isolated on its strand: the read's 50 bases are in the chromosome vector of '+', none in that of '-' outside M
    assert out['+'][0].indices.tolist() == list(range(210, 260)) and out['-'][0].indices.tolist() == list(range(220, 270))
    # reverse swaps the two strands' answers: the rows it calls '+' are the rows forward calls '-'
    fwd = dr.row_sense(reads.flag.values, reads.qname.tolist(), False, 'forward')
    swapped = _stranded_counts(reads, ['-' if s == '+' else '+' for s in fwd], chrom_len, parts)
    for s in sc.STRANDS:
        ro.assert_same(swapped[s], got['reverse'][s], 'swapped ' + s)


# --- against the restatement ----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def cases():
    """{(paired, n_rows, senses): (case, parts, {strand: restatement})}, computed once and not changed by any test."""
    out = {}
    for paired in (False, True):
        for n in ROW_COUNTS:
            for senses in (('mixed',) if n not in (65, None) else ('mixed', 'plus', 'minus')):
                case = sc.stranded_case(SEED, paired, n, senses)
                reads, sense, chrom_len, gene_df, exon_df, strand_of = case
                parts = sc.split_tables(gene_df, exon_df, strand_of)
                assert list(parts) == ['+', '-']
                out[paired, n, senses] = (case, parts, {s: sc.expected(reads, sense, chrom_len, parts, s, paired) for s in sc.STRANDS})
    return out


KEYS = [(paired, n, senses) for paired in (False, True) for n in ROW_COUNTS
        for senses in (('mixed',) if n not in (65, None) else ('mixed', 'plus', 'minus'))]


@pytest.mark.parametrize('paired,n_rows,senses', KEYS)
def test_device_equals_restatement_on_each_strand(paired, n_rows, senses, cases):
    (reads, sense, chrom_len, gene_df, exon_df, strand_of), parts, want = cases[paired, n_rows, senses]
    assert n_rows is None or len(reads) == n_rows
    got = _stranded_counts(reads, sense, chrom_len, parts, paired)
    for s in sc.STRANDS:
        ro.assert_same(got[s], want[s], '{0} {1} {2} strand {3}'.format(paired, n_rows, senses, s))
    if senses != 'mixed':                                      # nothing reaches the strand no row belongs to
        idle = '-' if senses == 'plus' else '+'
        assert sum(got[idle][2].values()) == 0 and got[idle][0] is None
    if n_rows is None:
        assert sum(sum(want[s][2].values()) for s in sc.STRANDS) > 200


def test_whole_case_counts_differ_from_unstranded_and_disagreeing_pairs_count_nowhere(cases):
    (reads, sense, chrom_len, gene_df, exon_df, strand_of), parts, want = cases[True, None, 'mixed']
    plain = ro.restate(reads, chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df, True)[2]
    stranded = dict(want['+'][2], **want['-'][2])
    assert sum(stranded[g] != plain[g] for g in plain) * 4 >= len(plain)
    # pairs whose mates disagree: taking their rows away changes nothing on either strand
    bad = set(sc.disagreeing_pairs(reads, sense))
    assert len(bad) >= 20
    keep = ~reads['qname_unpaired'].isin(bad).values
    got = _stranded_counts(reads[keep], sense[keep], chrom_len, parts, True)
    for s in sc.STRANDS:
        ro.assert_same(got[s], want[s], 'without the disagreeing pairs, strand ' + s)
    # ... while the same rows given one sense are counted
    agree = np.array(sense, dtype=object)
    first = {}
    for k, q in enumerate(reads['qname_unpaired']):
        agree[k] = first.setdefault(q, agree[k])
    both = _stranded_counts(reads, agree, chrom_len, parts, True)
    assert sum(sum(both[s][2].values()) for s in sc.STRANDS) > sum(sum(want[s][2].values()) for s in sc.STRANDS)


@pytest.mark.parametrize('paired', [False, True])
def test_a_strand_without_genes(paired):
    reads, sense, chrom_len, gene_df, exon_df, strand_of = sc.stranded_case(SEED, paired, 257, one_strand=True)
    parts = sc.split_tables(gene_df, exon_df, strand_of)
    assert list(parts) == ['+'] and set(sense) == {'+', '-'}
    got = _stranded_counts(reads, sense, chrom_len, parts, paired)
    ro.assert_same(got['+'], sc.expected(reads, sense, chrom_len, parts, '+', paired), 'the strand with genes')
    assert sum(got['+'][2].values()) > 0
    # the other strand is skipped by its callers; asked anyway, with no gene, it counts nothing
    none = gene_df.iloc[:0], exon_df.iloc[:0]
    csr, ol, counts = dr.chromosome_coverage_read_counts_df(reads, chrom_len, {'overlap_genes': [], 'isolated_genes': []}, none[0], none[1],
                                                            paired, sense=sense, strand='-')
    assert csr is None and ol == {} and counts == {}


def test_stranded_call_is_byte_identical_run_to_run(cases):
    (reads, sense, chrom_len, gene_df, exon_df, strand_of), parts, _ = cases[True, None, 'mixed']
    a = _stranded_counts(reads, sense, chrom_len, parts, True)
    b = _stranded_counts(reads, sense, chrom_len, parts, True)
    for s in sc.STRANDS:
        ro.assert_same(a[s], b[s], s)
