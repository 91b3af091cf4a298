"""
CPU tests of the full restatement of the reads -> coverage rules (tests/_reads_oracle.py), the oracle of
tests/test_gpu_reads_edges.py: it reproduces the reference's own outputs on every committed case (tests/golden/reads.npz:
se, pe, qi; tests/golden/reads_edges.npz: e00 ...), the committed cases reach every branch its census names, and the seeded
generators of tests/_reads_fixtures.py still give the cases the census was committed for and the variety the GPU tests'
fresh seeds rely on.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_fixtures as rf                                   # noqa: E402
import _reads_oracle as ro                                     # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_reads import _case, _expect                      # noqa: E402
from degnorm_amd import reads as dr                            # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure  # noqa: E402

# layout seeds of the GPU tests' fresh cases (the golden file holds seeds 0-5); what they are chosen for is asserted in
# test_fresh_seeds_reach_every_branch_and_annotation_shape
FRESH_SEEDS = (9, 10, 13, 14, 15, 17, 18, 29)
VARIANT_SEED = 7
# census keys that must be reached by the fresh single-end cases, and in addition by the paired ones
FRESH_MINIMA = ('empty_segment', 'negative_bound', 'wrap_only_piece', 'caught_2plus', 'iso_on_gene_last_base',
                'iso_spans_touching_genes', 'exon_drop', 'caught_0', 'caught_1', 'wrap', 'iso_union_drop')
FRESH_MINIMA_PAIRED = ('clip_left_resorted', 'clip_left_changed', 'clip_right_changed', 'pair_not_adjacent', 'pair_id_once',
                       'pair_id_thrice', 'ol_runs_merged', 'iso_runs_merged')
# keys no case can reach: negative units are taken out of the reference's cases; iso_gap_drop is a dead branch (see the oracle)
NEVER_IN_GOLDEN = ('negative_bound', 'iso_gap_drop')


def edge_keys(z):
    return sorted(k[:-len('_census')] for k in z.files if k.endswith('_census') and k != 'census_keys')


def reference_outputs(z, key):
    """The golden's reference outputs in the form restate returns."""
    from scipy import sparse
    has, idx, val, ol, counts = _expect(z, key)
    n = int(z[key + '_chrom_len'])
    csr = sparse.csr_matrix((val, idx, np.array([0, idx.size], dtype=np.int32)), shape=(1, n)) if has else None
    return csr, ol, counts


def frames(layout):
    chrom, chrom_len, genes = layout
    gene_df, exon_df = rf.tables(chrom, genes)
    return chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df


def fresh_case(seed, paired, variant=None):
    """(reads, chrom_len, overlap structure, gene_df, exon_df) of one fresh seeded case."""
    df, layout = rf.edge_case(seed, paired, variant=variant)
    return (df,) + frames(layout)


@pytest.mark.parametrize('key', ['se', 'pe', 'qi'])
def test_restatement_equals_reference_on_the_golden_layout(key):
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    got = ro.restate(reads, chrom_len, ov, gene_df, exon_df, paired)
    ro.assert_same(got, reference_outputs(z, key), key)
    assert got[3]['negative_bound'] == 0


def test_restatement_equals_reference_on_every_edge_case():
    z = golden('reads_edges')
    keys = edge_keys(z)
    assert len(keys) >= 12 and keys[0] == 'e00'
    names = z['census_keys'].tolist()
    assert names == list(ro.CENSUS_KEYS)
    n_paired = 0
    for key in keys:
        reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
        n_paired += paired
        got = ro.restate(reads, chrom_len, ov, gene_df, exon_df, paired)
        ro.assert_same(got, reference_outputs(z, key), key)
        assert [got[3][c] for c in names] == z[key + '_census'].tolist(), key       # the census committed with the case
    assert 4 <= n_paired <= len(keys) - 4


def test_committed_census_reaches_every_branch():
    z = golden('reads_edges')
    names = z['census_keys'].tolist()
    total = ro.merge_census(dict(zip(names, z[k + '_census'].tolist())) for k in edge_keys(z))
    print(dict(total))
    for c in ro.CENSUS_KEYS:
        if c in NEVER_IN_GOLDEN:
            assert total[c] == 0, c
        else:
            assert total[c] > 0, c
    assert total['nseg_max'] >= 4 and total['nseg_max'] == rf.reads_max_seg()
    # the two missing-stage variants are among the cases
    shapes = set()
    for k in edge_keys(z):
        grp = z[k + '_group']
        shapes.add((bool((grp >= 0).any()), bool((grp < 0).any())))
    assert shapes == {(True, True), (True, False), (False, True)}


def test_iso_gap_branch_is_dead_by_construction():
    """
    Why no case reaches iso_gap_drop: a unit gets there with [pos, end_pos] inside the union of the isolated genes' spans,
    and that union consists of exactly the genes' own positions (touching spans merge, nothing is added), so pos lies in a
    gene.  Checked on the packed intervals of every fresh layout: each position of iso_union is in one iso_iv span.
    """
    for seed in FRESH_SEEDS:
        chrom, chrom_len, genes = rf.random_layout(seed)
        gene_df, exon_df = rf.tables(chrom, genes)
        ann = dr.Annotation(chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df)
        in_union, in_gene = np.zeros(chrom_len, dtype=int), np.zeros(chrom_len, dtype=int)
        for a, b in ann.iso_union.tolist():
            in_union[a:b + 1] += 1
        for a, b in ann.iso_iv.tolist():
            in_gene[a:b + 1] += 1
        assert in_union.max(initial=0) <= 1 and np.array_equal(in_union, in_gene), seed


def test_negative_bound_rule_by_hand():
    """`0M10M` at 0 has the bounds [0, -1, -1, 8]: the unit is dropped and counted, single-end and as either mate."""
    layout = ('c', 400, [('a', [(1, 200)]), ('b', [(301, 380)])])
    chrom_len, ov, gene_df, exon_df = frames(layout)
    assert dr.cigar_segment_bounds('0M10M', 0) == [0, -1, -1, 8]
    se = rf._append(rf.synth_reads(0, layout, 0, skip=()), [[(0, '0M10M')], [(0, '10M')], [(1, '0M10M')]], False)
    csr, ol, counts, census = ro.restate(se, chrom_len, ov, gene_df, exon_df, False)
    assert census['negative_bound'] == 1 and counts == {'a': 2, 'b': 0}
    pe = rf._append(rf.synth_pairs(0, layout, 0, skip=()), [[(0, '30M'), (5, '10M')], [(5, '10M'), (0, '30M')],
                                                            [(1, '30M'), (5, '10M')]], True)
    csr, ol, counts, census = ro.restate(pe, chrom_len, ov, gene_df, exon_df, True)
    # mate 2 inside a mate 1 at 0 is clipped to -1; the other order clips mate 2 (at 0) to the right of mate 1; from 1 on
    # the clipped bounds are 0
    assert census['negative_bound'] == 1 and counts == {'a': 2, 'b': 0}


def test_generators_are_seeded_and_cover_the_variants():
    a, la = rf.edge_case(3, True)
    b, lb = rf.edge_case(3, True)
    assert la == lb and a.equals(b)
    n_first, n_last, shapes = 0, 0, set()
    for seed in range(12):
        chrom, chrom_len, genes = rf.random_layout(seed)
        assert 4 <= len(genes) <= 14 and chrom_len < 10000 and all(1 <= len(e) <= 4 for _, e in genes)
        gene_df, _ = rf.tables(chrom, genes)
        ov = get_gene_overlap_structure(gene_df)
        n_first += int(gene_df.gene_start.min() == 1)
        n_last += int(gene_df.gene_end.max() == chrom_len)
        shapes.add((len(ov['overlap_genes']), len(ov['isolated_genes'])))
    assert 0 < n_first < 12 and 0 < n_last < 12 and len(shapes) >= 6
    for seed in range(6):
        for variant, empty in (('groups_only', 'isolated_genes'), ('isolated_only', 'overlap_genes')):
            chrom, chrom_len, genes = rf.random_layout(seed, variant)
            ov = get_gene_overlap_structure(rf.tables(chrom, genes)[0])
            assert not ov[empty] and len(genes) >= 4, (seed, variant)


def test_fresh_seeds_reach_every_branch_and_annotation_shape():
    """The GPU tests' fresh cases, by the restatement alone: the census minima they assert, and the annotation shapes."""
    assert not set(FRESH_SEEDS) & set(range(6)) and len(FRESH_SEEDS) >= 8
    n_groups, n_union, group_size, first, last = [], [], [], 0, 0
    for seed in FRESH_SEEDS:
        chrom, chrom_len, genes = rf.random_layout(seed)
        gene_df, exon_df = rf.tables(chrom, genes)
        ov = get_gene_overlap_structure(gene_df)
        ann = dr.Annotation(chrom_len, ov, gene_df, exon_df)
        n_groups.append(len(ann.group_iv))
        n_union.append(len(ann.iso_union))
        group_size += [len(g) for g in ov['overlap_genes']]
        first += int(gene_df.gene_start.min() == 1)
        last += int(exon_df.end.max() == chrom_len)
    assert max(n_groups) > 2 and min(n_groups) == 0 and max(n_union) > 3 and min(n_union) == 0
    assert max(group_size) > 3 and first >= 2 and last >= 2
    for paired in (False, True):
        total = ro.merge_census(ro.restate(*fresh_case(seed, paired), paired)[3] for seed in FRESH_SEEDS)
        print('paired' if paired else 'single-end', dict(total))
        for c in FRESH_MINIMA + (FRESH_MINIMA_PAIRED if paired else ()):
            assert total[c] > 0, (paired, c)
        assert total['iso_gap_drop'] == 0 and total['nseg_max'] == rf.reads_max_seg()
