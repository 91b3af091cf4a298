"""
CPU tests of the reads -> coverage / read counts layer (degnorm_amd.reads, degnorm_amd.gene_processing): the host CIGAR and
inclusion helpers against the reference's goldens (tests/golden/reads.npz), the overlap partition, the annotation packing,
and the errors the reference raises.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_fixtures as rf                                   # noqa: E402
from conftest import golden                                    # noqa: E402
from degnorm_amd import reads as dr                            # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure  # noqa: E402


def _cigars(z, key):
    off, buf = z[key + '_cig_off'], z[key + '_cig'].tobytes()
    return [buf[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


def test_cigar_segment_bounds_matches_reference_fuzz():
    z = golden('reads')
    cig, pos, nseg = _cigars(z, 'fz'), z['fz_pos'], z['fz_nseg']
    bounds, k = z['fz_bounds'], 0
    assert (nseg == 0).any() and len(cig) >= 2000
    for c, s, n, e in zip(cig, pos.tolist(), nseg.tolist(), z['fz_end_pos'].tolist()):
        if n == 0:
            with pytest.raises(ValueError):
                dr.cigar_segment_bounds(c, s)
        else:
            assert dr.cigar_segment_bounds(c, s) == bounds[k:k + 2 * n].tolist(), c
        k += 2 * n
        assert s + dr.cigar_length(c) == e


def test_cigar_semantics_by_hand():
    assert dr.cigar_segment_bounds('50M25N50M', 100) == [100, 149, 175, 224]
    assert dr.cigar_segment_bounds('5S10M', 0) == [5, 14]              # a soft clip shifts the read
    assert dr.cigar_segment_bounds('10M5=10M', 0) == [0, 9, 15, 24]     # '=' is a non-M op, one more after an M
    assert dr.cigar_segment_bounds('10M10M', 0) == [0, 9, 9, 18]
    with pytest.raises(ValueError, match='no matching region'):
        dr.cigar_segment_bounds('10S5I', 7)


def test_fill_in_bounds():
    assert dr.fill_in_bounds([10, 13, 20, 24]).tolist() == [10, 11, 12, 20, 21, 22, 23]
    assert dr.fill_in_bounds([10, 13, 20, 21], endpoint=True).tolist() == [10, 11, 12, 13, 20, 21]
    with pytest.raises(ValueError):
        dr.fill_in_bounds([1, 2, 3])


def test_determine_full_inclusion():
    f = dr.BamReadsProcessor.determine_full_inclusion
    assert f([10, 32, 45, 90], [[[8, 40], [44, 100]], [[2, 20], [60, 400]]]) == [0]
    assert f([10, 12], [[[8, 40]], [[10, 12]], [[11, 40]]]) == [0, 1]
    assert f([50, 49], [[[60, 70]], [[0, 48]]]) == []                    # an empty segment still compares by raw values
    assert f([50, 49], [[[40, 70]]]) == [0]


def _brute_partition(gene_df):
    lo, hi = gene_df.gene_start.values - 1, gene_df.gene_end.values
    n = len(lo)
    parent = list(range(n))

    def root(i):
        while parent[i] != i:
            i = parent[i]
        return i
    for i in range(n):
        for j in range(n):
            if lo[i] < hi[j] and lo[j] < hi[i]:
                parent[root(i)] = root(j)
    comps = {}
    for i in range(n):
        comps.setdefault(root(i), []).append(gene_df.gene.values[i])
    return sorted(sorted(c) for c in comps.values() if len(c) > 1), sorted(c[0] for c in comps.values() if len(c) == 1)


def test_overlap_structure_golden_layouts():
    for layout in (rf.golden_layout(), rf.quiet_layout()):
        gene_df, _ = rf.tables(*layout[::2])
        ov = get_gene_overlap_structure(gene_df)
        groups, iso = _brute_partition(gene_df)
        assert sorted(sorted(g) for g in ov['overlap_genes']) == groups
        assert sorted(ov['isolated_genes']) == iso
    gene_df, _ = rf.tables(*rf.golden_layout()[::2])
    ov = get_gene_overlap_structure(gene_df)
    assert ov == {'overlap_genes': [['A', 'B', 'C'], ['D', 'E']], 'isolated_genes': ['F', 'G', 'H', 'I']}


def test_overlap_structure_by_hand():
    df = pd.DataFrame({'gene': ['W', 'M', 'R', 'E', 'T1', 'T2', 'X', 'Y', 'Z'],
                       'gene_start': [100, 150, 215, 600, 1000, 1101, 2000, 1990, 2300],
                       'gene_end': [200, 230, 280, 822, 1100, 1200, 2100, 2000, 2400]})
    ov = get_gene_overlap_structure(df)
    # W - M - R chain; T1 / T2 touch (1100 | 1101) and stay isolated; Y ends on X's first base: they overlap
    assert ov == {'overlap_genes': [['W', 'M', 'R'], ['X', 'Y']], 'isolated_genes': ['E', 'T1', 'T2', 'Z']}
    rng = np.random.default_rng(0)
    s = rng.integers(1, 5000, size=300)
    df = pd.DataFrame({'gene': ['g{0}'.format(i) for i in range(300)], 'gene_start': s, 'gene_end': s + rng.integers(0, 60, size=300)})
    ov = get_gene_overlap_structure(df)
    groups, iso = _brute_partition(df)
    assert sorted(sorted(g) for g in ov['overlap_genes']) == groups and sorted(ov['isolated_genes']) == iso
    first = [df.gene.tolist().index(g[0]) for g in ov['overlap_genes']]
    assert first == sorted(first)


def test_annotation_packing():
    chrom, chrom_len, genes = rf.golden_layout()
    gene_df, exon_df = rf.tables(chrom, genes)
    ann = dr.Annotation(chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df)
    assert ann.group_iv.tolist() == [[100, 1199], [2000, 2999]]
    assert ann.iso_union.tolist() == [[3200, 3899], [4000, 4399], [5000, 5199]]     # F and G touch: one interval
    assert ann.exon_iv[:3].tolist() == [[100, 349], [500, 999], [1100, 1199]]
    d = ann.ol_names.index('D')
    e = ann.ol_exon[ann.ol_exon_off[d]:ann.ol_exon_off[d + 1]].tolist()
    assert e == [[2000, 2300], [2100, 2600], [2700, 2800]]                         # starts and ends sorted separately
    with pytest.raises(ValueError, match='does not match'):
        dr.Annotation(chrom_len, {'overlap_genes': [], 'isolated_genes': ['A']}, gene_df, exon_df)


def test_bam_processor_needs_pysam(tmp_path):
    try:
        import pysam  # noqa: F401
        pytest.skip('pysam is installed')
    except ImportError:
        pass
    bam = tmp_path / 's.bam'
    bam.write_bytes(b'')
    (tmp_path / 's.bam.bai').write_bytes(b'')
    with pytest.raises(ImportError, match='pysam'):
        dr.BamReadsProcessor(str(bam), str(bam) + '.bai')


def test_file_skip_rule_needs_no_device(tmp_path):
    """All files present: nothing is loaded or computed (reads.py:374-386)."""
    chrom, chrom_len, genes = rf.golden_layout()
    gene_df, exon_df = rf.tables(chrom, genes)
    p = dr.BamReadsProcessor.__new__(dr.BamReadsProcessor)
    p.sample_id, p.save_dir, p.verbose, p.paired = 's1', str(tmp_path), False, False

    def boom(c):
        raise AssertionError('reads loaded although every file exists')
    p.load_chromosome_reads = boom
    for f in p._files(chrom):
        open(f, 'w').close()
    assert p.chromosome_coverage_read_counts(get_gene_overlap_structure(gene_df), gene_df, exon_df, chrom) is None
