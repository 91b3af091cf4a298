"""
GPU test of the BAM + GTF pipeline (degnorm_amd.pipeline, `python -m degnorm_amd`) against the reference's chain on the
same annotation and the same seeded reads (tests/golden/pipeline.npz, made by tests/golden/make_golden_pipeline.py): three
single-end samples on two chromosomes, one BAM reference the annotation lacks, one annotated chromosome no BAM has.
The pipeline adds no arithmetic between the reads and the NMF-OA input, so everything up to that input is compared for
equality; the NMF-OA results are compared for equality with a GeneNMFOA run on the golden's own matrices and counts
(two runs of the device path on the same input are bit-identical, tests/test_gpu_parity.py).
"""
import os
import pickle
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                             # noqa: E402
import _gtf_fixtures as gf                                             # noqa: E402
from conftest import golden, GOLDEN                                    # noqa: E402
from test_annotation_host import RUN_COLS, assert_same_table, golden_frame     # noqa: E402
from degnorm_amd import warm_start                                     # noqa: E402
from degnorm_amd.nmf import GeneNMFOA                                  # noqa: E402
from degnorm_amd.pipeline import prepare_inputs, run_pipeline          # noqa: E402

pytestmark = pytest.mark.gpu

GTF = os.path.join(GOLDEN, 'pipeline.gtf')
RESULT_FILES = ['degradation_index_scores.csv', 'adjusted_read_counts.csv', 'ran_baseline_selection.csv']
ITER, NMF_ITER = 3, 50


@pytest.fixture(scope='module')
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp('bams')
    paths = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(d / (s + '.bam'))
        bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1))
        paths.append(p)
    return paths, [p + '.bai' for p in paths]


def golden_inputs(z, dropped):
    """The reference's coverage dict, gene table and read counts without the genes its filter drops."""
    samples = z['sample_ids'].tolist()
    genes, lens = z['cov_genes'].tolist(), z['cov_len']
    off = np.r_[0, np.cumsum(lens * len(samples))]
    cov = OrderedDict((g, z['cov_flat'][off[k]:off[k + 1]].reshape(len(samples), lens[k])) for k, g in enumerate(genes) if g not in dropped)
    genes_df = golden_frame(z, 'genes', ['gene', 'chr', 'gene_start', 'gene_end'])
    counts_df = golden_frame(z, 'read_counts', ['gene', 'chr'] + samples)
    keep = ~genes_df.gene.isin(dropped)
    return cov, genes_df[keep].reset_index(drop=True), counts_df[keep.values].reset_index(drop=True), samples


def assert_same_cov(got, expect):
    assert list(got) == list(expect)
    for g in expect:
        assert got[g].dtype == np.float64 and got[g].shape == expect[g].shape
        np.testing.assert_array_equal(got[g], expect[g])


def test_run_pipeline_equals_reference_chain(bams, tmp_path):
    z = golden('pipeline')
    bam_files, bai_files = bams
    out = str(tmp_path / 'out')
    os.makedirs(out)
    minimax = int(z['case_a_minimax'])
    dropped = z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    assert len(dropped) >= 1 and len(cov_e) >= 6

    model, estimates, cov, counts_df, genes_df, exon_df, sample_ids = run_pipeline(
        bam_files, bai_files, GTF, out, degnorm_iter=ITER, nmf_iter=NMF_ITER, minimax_coverage=minimax, verbose=False)

    # up to the NMF-OA input: tables, dict order, matrices
    assert sample_ids == samples == gf.PIPELINE_SAMPLES
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_cov(cov, cov_e)
    # what it leaves on disk: the two tables before the filter, a pickle per chromosome, no per-sample directories
    all_cov, all_genes, all_counts, _ = golden_inputs(z, [])
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'gene_exon_metadata.csv')),
                                  golden_frame(z, 'exon', RUN_COLS).reset_index(drop=True))
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'read_counts.csv')), all_counts)
    for c in z['chroms'].tolist():
        with open(os.path.join(out, c, 'coverage_matrices_{0}.pkl'.format(c)), 'rb') as f:
            chrom_cov = pickle.load(f)
        assert type(chrom_cov) is dict
        assert_same_cov(chrom_cov, OrderedDict((g, all_cov[g]) for g in z['pkl_{0}_genes'.format(c)].tolist()))
    assert not any(os.path.exists(os.path.join(out, s)) for s in samples)
    assert not os.path.exists(os.path.join(out, 'chr7')) and not os.path.exists(os.path.join(out, 'chrM'))

    # the NMF-OA run: what GeneNMFOA gives on the golden's own input with the same parameters
    ref = GeneNMFOA(degnorm_iter=ITER, nmf_iter=NMF_ITER)
    est_e = ref.run(cov_e, reads_dat=counts_e[samples].values.astype(np.float64))
    assert model.genes == ref.genes == list(cov_e)
    np.testing.assert_array_equal(model.rho, ref.rho)
    np.testing.assert_array_equal(model.x_adj, ref.x_adj)
    np.testing.assert_array_equal(model.ran_baseline_selection, ref.ran_baseline_selection)
    for a, b in zip(estimates, est_e):
        np.testing.assert_array_equal(a, b)
    di = pd.read_csv(os.path.join(out, RESULT_FILES[0]))
    assert di.gene.tolist() == list(cov_e) and di.columns.tolist() == ['chr', 'gene'] + samples
    np.testing.assert_allclose(di[samples].values, ref.rho, rtol=1e-12, atol=0)              # the CSV's decimal round trip

    # the directory is a warm-start directory
    dat = warm_start.load_from_previous(out)
    assert_same_cov(dat['gene_cov_dict'], all_cov)
    assert dat['sample_ids'] == samples
    pd.testing.assert_frame_equal(dat['genes_df'], all_genes)
    pd.testing.assert_frame_equal(dat['read_count_df'], all_counts)

    # the command in a child process writes the same result files
    out_cli = str(tmp_path / 'cli_out')
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd', '--bam-files'] + bam_files + ['--bai-files'] + bai_files +
                       ['-g', GTF, '-o', out_cli, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    for name in RESULT_FILES + ['gene_exon_metadata.csv', 'read_counts.csv']:
        with open(os.path.join(out, name), 'rb') as fa, open(os.path.join(out_cli, name), 'rb') as fb:
            assert fa.read() == fb.read(), name
    assert os.path.isfile(os.path.join(out_cli, 'degnorm.log'))
    # and -w on the first directory takes the warm-start path to the same scores
    out_warm = str(tmp_path / 'warm_out')
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd', '-w', out, '-o', out_warm, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER),
                        '--minimax-coverage', str(minimax)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    for name in RESULT_FILES:
        with open(os.path.join(out, name), 'rb') as fa, open(os.path.join(out_warm, name), 'rb') as fb:
            assert fa.read() == fb.read(), name


def test_prepare_inputs_filter_by_length(bams, tmp_path):
    """Filter case B: no coverage bound, a take-every equal to the shortest gene.  No NMF-OA run here: with a take-every above
    1 GeneNMFOA draws its sample offsets from np.random, so two runs are not comparable."""
    z = golden('pipeline')
    bam_files, bai_files = bams
    out = str(tmp_path / 'out')
    os.makedirs(out)
    rate = int(z['case_b_downsample'])
    dropped = z['case_b_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    assert len(dropped) >= 1 and len(cov_e) >= 2
    cov, counts_df, genes_df, exon_df, sample_ids = prepare_inputs(bam_files, bai_files, GTF, out, downsample_rate=rate,
                                                                   minimax_coverage=0, verbose=False)
    assert sample_ids == samples
    assert_same_cov(cov, cov_e)
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert min(m.shape[1] for m in cov.values()) > rate


def test_no_gene_left_is_the_reference_error(bams, tmp_path):
    bam_files, bai_files = bams
    out = str(tmp_path / 'out')
    os.makedirs(out)
    with pytest.raises(ValueError, match='No genes available to run through DegNorm!'):
        prepare_inputs(bam_files, bai_files, GTF, out, minimax_coverage=10 ** 9, verbose=False)
