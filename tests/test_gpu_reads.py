"""
GPU tests of dn_read_coverage (csrc/dn_reads.hip) through degnorm_amd.reads: single-end and paired outputs equal the
reference's goldens exactly (tests/golden/reads.npz), the files BamReadsProcessor writes, the device CIGAR parser against
the reference's fuzz goldens, and a 2 M-read / 20 Mb scale case against the numpy restatement in tests/_reads_fixtures.py,
bit-identical from run to run.
"""
import os
import pickle
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_fixtures as rf                                   # noqa: E402
from conftest import golden                                    # noqa: E402
from degnorm_amd import reads as dr                            # noqa: E402

pytestmark = pytest.mark.gpu


def _case(z, key):
    off, buf = z[key + '_cig_off'], z[key + '_cig'].tobytes()
    reads = pd.DataFrame({'pos': z[key + '_pos'], 'cigar': [buf[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]})
    paired = key + '_pair' in z.files
    if paired:
        reads['qname_unpaired'] = z[key + '_pair']
    genes = z[key + '_gene'].tolist()
    gene_df = pd.DataFrame({'chr': 'c', 'gene': genes, 'gene_start': z[key + '_gene_start'], 'gene_end': z[key + '_gene_end']})
    exon_df = pd.DataFrame({'chr': 'c', 'gene': z[key + '_exon_gene'].tolist(), 'start': z[key + '_exon_start'],
                            'end': z[key + '_exon_end']}).merge(gene_df, on=['chr', 'gene'])
    grp = z[key + '_group']
    ov = {'overlap_genes': [[g for g, k in zip(genes, grp) if k == j] for j in range(grp.max() + 1)],
          'isolated_genes': [g for g, k in zip(genes, grp) if k < 0]}
    return reads, int(z[key + '_chrom_len']), ov, gene_df, exon_df, paired


def _expect(z, key):
    names, off = z[key + '_ol_gene'].tolist(), z[key + '_ol_off']
    ol = {g: z[key + '_ol_cov'][off[i]:off[i + 1]] for i, g in enumerate(names)}
    counts = dict(zip(z[key + '_gene'].tolist(), z[key + '_counts'].tolist()))
    return bool(z[key + '_has_csr']), z[key + '_csr_idx'], z[key + '_csr_val'], ol, counts


def _check(csr, ol, counts, exp):
    has, idx, val, ol_e, counts_e = exp
    assert (csr is not None) == has
    if has:
        assert csr.dtype == np.int64 and csr.indices.dtype == np.int32 and csr.shape[0] == 1
        np.testing.assert_array_equal(csr.indices, idx)
        np.testing.assert_array_equal(csr.data, val)
    assert list(ol) == list(ol_e)
    for g in ol_e:
        assert ol[g].dtype == np.int64
        np.testing.assert_array_equal(ol[g], ol_e[g], err_msg=g)
    assert counts == counts_e


@pytest.mark.parametrize('key', ['se', 'pe', 'qi'])
def test_device_matches_reference_golden(key):
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    csr, ol, counts = dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, paired)
    _check(csr, ol, counts, _expect(z, key))
    assert list(counts) == gene_df.gene.tolist()


@pytest.mark.parametrize('key', ['se', 'pe', 'qi'])
def test_bam_processor_files_match_golden(key, tmp_path):
    from scipy import sparse
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    p = dr.BamReadsProcessor.__new__(dr.BamReadsProcessor)
    p.header = pd.DataFrame({'chr': ['c'], 'length': [chrom_len]})
    p.paired, p.sample_id, p.save_dir, p.verbose = paired, 's1', str(tmp_path), False
    calls = []
    p.load_chromosome_reads = lambda c: calls.append(c) or reads.copy()
    p.chromosome_coverage_read_counts(ov, gene_df, exon_df, 'c')
    f_csr, f_ol, f_cnt = p._files('c')
    has = bool(z[key + '_has_csr'])
    assert os.path.isfile(f_csr) == has                      # no chrom_coverage file when no read is isolated (:711)
    csr = sparse.load_npz(f_csr) if has else None
    with open(f_ol, 'rb') as f:
        ol = pickle.load(f)
    cnt = pd.read_csv(f_cnt)
    assert list(cnt.columns) == ['gene', 's1']
    _check(csr, ol, dict(zip(cnt.gene, cnt.s1.astype(int))), _expect(z, key))
    # skip-if-present: the files are kept and nothing is recomputed; with the npz missing (the chromosome has isolated genes,
    # so it needs one) it runs again -- also when the run wrote none because no read reached the isolated stage (:374-376)
    p.chromosome_coverage_read_counts(ov, gene_df, exon_df, 'c')
    assert calls == (['c'] if has else ['c', 'c'])
    if has:
        os.remove(f_csr)
        p.chromosome_coverage_read_counts(ov, gene_df, exon_df, 'c')
        assert calls == ['c', 'c'] and os.path.isfile(f_csr)


def test_device_cigar_parser_matches_reference_fuzz():
    z = golden('reads')
    off, buf = z['fz_cig_off'], z['fz_cig'].tobytes()
    cig = [buf[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]
    out, end_pos = dr.device_cigar_bounds(cig, z['fz_pos'], max_seg=16)
    k = 0
    for r, n in enumerate(z['fz_nseg'].tolist()):
        if n == 0:
            assert out[r] is None, cig[r]
        else:
            assert out[r] == z['fz_bounds'][k:k + 2 * n].tolist(), cig[r]
        k += 2 * n
    np.testing.assert_array_equal(end_pos, z['fz_end_pos'])


def test_no_match_cigar_raises():
    chrom, chrom_len, genes = rf.golden_layout()
    gene_df, exon_df = rf.tables(chrom, genes)
    from degnorm_amd.gene_processing import get_gene_overlap_structure
    reads = pd.DataFrame({'pos': [150, 160], 'cigar': ['20M', '10S5I']})
    with pytest.raises(ValueError, match='no matching region'):
        dr.chromosome_coverage_read_counts_df(reads, chrom_len, get_gene_overlap_structure(gene_df), gene_df, exon_df, False)


def test_scale_against_restatement_and_run_to_run():
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case()
    idx_e, val_e, ol_e, counts_e = rf.restate_single_end(reads, chrom_len, ov, gene_df, exon_df)
    assert idx_e.size > 100000 and len(ol_e) > 100 and sum(counts_e.values()) > 1000000
    runs = []
    for _ in range(2):
        csr, ol, counts = dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, False)
        runs.append((csr, ol, counts))
    for csr, ol, counts in runs:
        np.testing.assert_array_equal(csr.indices, idx_e)
        np.testing.assert_array_equal(csr.data, val_e)
        assert counts == counts_e
        assert sorted(ol) == sorted(ol_e)
        for g in ol_e:
            np.testing.assert_array_equal(ol[g], ol_e[g], err_msg=g)
    (a, oa, ca), (b, ob, cb) = runs
    assert a.indices.tobytes() == b.indices.tobytes() and a.data.tobytes() == b.data.tobytes() and ca == cb
    assert all(oa[g].tobytes() == ob[g].tobytes() for g in oa)
