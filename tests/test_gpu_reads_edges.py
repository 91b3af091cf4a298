"""
GPU tests of the read-coverage kernel (k_reads, csrc/dn_reads.hip) and the host packing in front of it (reads.Annotation)
on random annotations and on the edges of the rules, against the reference's goldens (tests/golden/reads_edges.npz) and
against the full restatement of tests/_reads_oracle.py, which tests/test_reads_oracle_host.py holds to the reference:

  golden cases     e00 ...: random layouts, the groups-only and isolated-only variants, every read mutator, the segment cap
  fresh seeds      8 layouts x {single-end, paired} that are not in the golden file; the census of the restatement is
                   asserted to reach the branches the cases are there for (zero-length M ops and the re-sort of clipped
                   bounds, empty segments, bounds below 0, the wrap piece alone, interleaved pairs, reads over touching genes)
  forced variants  no isolated gene (csr is None) and no overlap group (an empty overlap dict)
  segment cap      DN_READS_MAX_SEG M ops per row and per mate with the wrap piece on top; one more is a ValueError
  BAM path         the fresh cases through NativeBamReadsProcessor, mates paired on the host and on the device
  run to run       byte-identical outputs

iso_gap_drop (`p > iso_iv[2 * ig + 1]` in the kernel) is not among the asserted minima: no input reaches it, see
test_reads_oracle_host.test_iso_gap_branch_is_dead_by_construction.  Its edge is asserted instead -- iso_on_gene_last_base,
reads that start on the last base of their gene, which a `>=` in its place would drop.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _pair_cases as pc                                       # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
import _reads_oracle as ro                                     # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_bam import _run, expected_frame                  # noqa: E402
from test_gpu_reads import _case, _check, _expect              # noqa: E402
from test_reads_oracle_host import (FRESH_MINIMA, FRESH_MINIMA_PAIRED, FRESH_SEEDS, VARIANT_SEED, edge_keys, frames,   # noqa: E402
                                    fresh_case)
from degnorm_amd import reads as dr                            # noqa: E402

pytestmark = pytest.mark.gpu

MAX_SEG = rf.reads_max_seg()
EDGE_KEYS = edge_keys(golden('reads_edges'))
FRESH = [(seed, paired) for seed in FRESH_SEEDS for paired in (False, True)]


@pytest.mark.parametrize('key', EDGE_KEYS)
def test_device_matches_reference_on_edge_golden(key):
    z = golden('reads_edges')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    csr, ol, counts = dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, paired)
    _check(csr, ol, counts, _expect(z, key))
    assert list(counts) == gene_df.gene.tolist()


@pytest.fixture(scope='module')
def fresh():
    """{(seed, paired): (case, restatement)} of the fresh cases, computed once and not changed by any test."""
    out = {}
    for seed, paired in FRESH:
        case = fresh_case(seed, paired)
        out[seed, paired] = (case, ro.restate(*case, paired))
    for paired in (False, True):
        total = ro.merge_census(out[seed, paired][1][3] for seed in FRESH_SEEDS)
        print('census of the fresh', 'paired' if paired else 'single-end', 'cases:', dict(total))
        for c in FRESH_MINIMA + (FRESH_MINIMA_PAIRED if paired else ()):
            assert total[c] > 0, (paired, c)
        assert total['nseg_max'] == MAX_SEG
    return out


@pytest.mark.parametrize('seed,paired', FRESH)
def test_device_equals_restatement_on_fresh_seed(seed, paired, fresh):
    case, want = fresh[seed, paired]
    got = dr.chromosome_coverage_read_counts_df(*case, paired)
    ro.assert_same(got, want, 'seed {0} paired {1}'.format(seed, paired))
    assert sum(want[2].values()) > 40                          # the case counts reads at all


@pytest.mark.parametrize('paired', [False, True])
@pytest.mark.parametrize('variant', ['groups_only', 'isolated_only'])
def test_missing_annotation_stage(variant, paired):
    case = fresh_case(VARIANT_SEED, paired, variant)
    want = ro.restate(*case, paired)
    csr, ol, counts = dr.chromosome_coverage_read_counts_df(*case, paired)
    ro.assert_same((csr, ol, counts), want, variant)
    assert sum(counts.values()) > 40
    if variant == 'groups_only':
        assert csr is None and len(ol) == len(counts) and not case[2]['isolated_genes']
    else:
        assert ol == {} and csr is not None and csr.nnz > 0 and not case[2]['overlap_genes']


# --- the segment cap ---------------------------------------------------------------------------------------------------

def _cap_call(reads, paired):
    return dr.chromosome_coverage_read_counts_df(reads, *frames(rf.cap_layout()), paired)


def _cap_normal_call_is_right():
    """After an error: an ordinary call in the same process gives the right answer."""
    for paired in (False, True):
        reads = rf.cap_reads(paired, MAX_SEG)
        ro.assert_same(_cap_call(reads, paired), ro.restate(reads, *frames(rf.cap_layout()), paired), 'after an error')


def test_rows_at_the_segment_cap_equal_restatement():
    layout = frames(rf.cap_layout())
    se = rf.cap_reads(False, MAX_SEG)
    assert [len(dr.cigar_segment_bounds(c, 0)) // 2 for c in se.cigar] == [MAX_SEG, MAX_SEG, 1]
    want = ro.restate(se, *layout, False)
    ro.assert_same(_cap_call(se, False), want, 'single-end')
    assert want[2]['K'] == 3 and want[3]['nseg_max'] == MAX_SEG and want[3]['wrap'] == 1
    pe = rf.cap_reads(True, MAX_SEG)
    want = ro.restate(pe, *layout, True)
    ro.assert_same(_cap_call(pe, True), want, 'paired')
    # the first pair: mate 1 on K's first base, 2 * MAX_SEG segments that all stay pieces, and the wrap piece
    assert want[2]['K'] == 3 and want[3]['wrap'] == 1 and want[3]['wrap_only_piece'] == 0
    first = ro.restate(pe.iloc[:2], *layout, True)
    k = first[1]['K']
    assert first[2]['K'] == 1 and int(k.sum()) == 2 * MAX_SEG + 1 and int(k.max()) == 1


def test_a_row_over_the_segment_cap_is_an_error():
    over, other = rf.cap_cigar(MAX_SEG + 1), rf.cap_cigar(MAX_SEG, first=3)
    assert len(dr.cigar_segment_bounds(over, 0)) // 2 == MAX_SEG + 1
    message = '{0} has more than {1} match segments \\(DN_READS_MAX_SEG\\)'
    se = pd.DataFrame({'pos': [300, 60, 320], 'cigar': ['30M', over, '30M']})
    with pytest.raises(ValueError, match=message.format(over, MAX_SEG)):
        _cap_call(se, False)
    _cap_normal_call_is_right()
    for cigars in ([over, other], [other, over]):              # as mate 1 and as mate 2: the message names the row over the cap
        pe = pd.DataFrame({'pos': [60, 200, 300, 320], 'cigar': cigars + ['30M', '30M'], 'qname_unpaired': ['b', 'b', 'a', 'a']})
        with pytest.raises(ValueError, match=message.format(over, MAX_SEG)):
            _cap_call(pe, True)
        _cap_normal_call_is_right()
    # outside the position pre-filter (before the first gene's start, K's base 50) the row is never parsed
    se_out = pd.DataFrame({'pos': [300, 40, 320], 'cigar': ['30M', over, '30M']})
    csr, ol, counts = _cap_call(se_out, False)
    assert counts == {'K': 2, 'L': 0, 'M': 0}
    pe_out = pd.DataFrame({'pos': [300, 40, 200, 320], 'cigar': ['30M', over, other, '30M'], 'qname_unpaired': ['a', 'b', 'b', 'a']})
    ro.assert_same(_cap_call(pe_out, True), ro.restate(pe_out, *frames(rf.cap_layout()), True), 'pre-filtered')
    # a kept row without M and a kept row over the cap: the reference's error comes first
    both = pd.DataFrame({'pos': [60, 300, 200], 'cigar': [over, '30M', '10S5I']})
    with pytest.raises(ValueError, match='CIGAR string 10S5I has no matching region'):
        _cap_call(both, False)
    _cap_normal_call_is_right()


# --- the BAM path ------------------------------------------------------------------------------------------------------

def _bam_outputs(files):
    csr, ol, cnt = files
    return csr, ol if ol is not None else {}, dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int)))


def _stable_frame(written, tid):
    """expected_frame with equal pair keys left in file order: the order pair='device' gives."""
    df = expected_frame(written, tid, True, False)
    df['qname_unpaired'] = df.qname.apply(lambda x: '.'.join(x.split('.')[:-1]))
    return df.sort_values('qname_unpaired', kind='stable')


@pytest.mark.parametrize('seed,paired', FRESH)
def test_bam_path_equals_restatement_on_fresh_seed(seed, paired, fresh, tmp_path):
    (reads, chrom_len, ov, gene_df, exon_df), _ = fresh[seed, paired]
    chrom = gene_df.chr.iloc[0]
    df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.values, 'cigar': reads.cigar.values, 'next_ref': 0})
    p = str(tmp_path / 's.bam')
    written, _, _ = bf.write_bam(p, [(chrom, chrom_len)], df, straddle=bool(seed % 2))
    assert any('0M' == c[:2] or 'M0' in c for c in written.cigar) and any('=' in c or 'X' in c for c in written.cigar)
    frame = expected_frame(written, 0, True, paired)
    want = ro.restate(frame, chrom_len, ov, gene_df, exon_df, paired)
    assert sum(want[2].values()) > 40
    proc, host = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'host', pair='host')
    assert proc.paired == paired
    ro.assert_same(_bam_outputs(host), want, 'host pairing')
    if not paired:
        return
    # mates paired on the device: equal keys stay in file order, so the frame is the stable sort of the same rows.  (In
    # files of this size pandas' quicksort always orders some overlapping pair differently -- order_sensitive_pairs counts
    # them -- so the host's frame is not the expectation here.)
    n_pairs, n_overlap, n_differ = pc.order_sensitive_pairs(written.qname.tolist(), written.pos.tolist(), written.cigar.tolist())
    print('pairs', n_pairs, 'with overlapping mates', n_overlap, 'ordered differently by the two sorts', n_differ)
    assert n_pairs > 80 and n_overlap > 20
    stable = ro.restate(_stable_frame(written, 0), chrom_len, ov, gene_df, exon_df, True)
    _, dev = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'device', pair='device')
    ro.assert_same(_bam_outputs(dev), stable, 'device pairing')


def test_paired_edge_case_is_byte_identical_run_to_run(fresh):
    case, _ = fresh[FRESH_SEEDS[1], True]
    a = dr.chromosome_coverage_read_counts_df(*case, True)
    b = dr.chromosome_coverage_read_counts_df(*case, True)
    assert a[0].indices.tobytes() == b[0].indices.tobytes() and a[0].data.tobytes() == b[0].data.tobytes()
    assert list(a[1]) == list(b[1]) and len(a[1]) > 0 and all(a[1][g].tobytes() == b[1][g].tobytes() for g in a[1])
    assert a[2] == b[2]
