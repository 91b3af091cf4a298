"""
Seeded DegNorm output directories for the data_access tests (tests/test_data_access_host.py, tests/test_gpu_text.py) and for
tests/golden/make_golden_data_access.py, which runs the real reference on the first one.

write_reference_dir   what the reference's own test_data_access.py builds: GENE_1 (225 bases) and GENE_2 (2 495 bases) on
                      chr1, two samples, the three .csv files and the two pickles -- seeded, and with estimates that are
                      not integers, so that the fifth decimal is rounded
write_hard_dir        lower-case gene names in the files, a second chromosome, a gene that only the raw pickle has, and a
                      sample id with a space in it
write_nan_dir         three genes, one of which holds a NaN in its estimate and an infinity in its raw coverage
"""
import os
import pickle

import numpy as np
from pandas import DataFrame

REFERENCE_GENES = ['GENE_1', 'GENE_2']
REFERENCE_SAMPLES = ['sample_1', 'sample_2']
HARD_SAMPLES = ['s 1', 's2', 's3']


def _write(outdir, exon_rows, sample_ids, raw, est):
    """exon_rows: (chr, start, end, gene); raw / est: {chr: {gene: p x L matrix}}."""
    os.makedirs(outdir, exist_ok=True)
    exon_df = DataFrame(exon_rows, columns=['chr', 'start', 'end', 'gene'])
    exon_df['exon_id'] = np.arange(len(exon_df))
    exon_df['gene_end'] = exon_df.groupby('gene').end.transform('max')
    exon_df['gene_start'] = exon_df.groupby('gene').start.transform('min')
    exon_df.to_csv(os.path.join(outdir, 'gene_exon_metadata.csv'), index=False)
    genes = exon_df.drop_duplicates('gene')
    di = DataFrame({'chr': genes.chr.values, 'gene': genes.gene.values})
    for k, s in enumerate(sample_ids):
        di[s] = np.round(np.linspace(0.05, 0.6, len(di)) + 0.01 * k, 4)
    di.to_csv(os.path.join(outdir, 'degradation_index_scores.csv'), index=False)
    di.to_csv(os.path.join(outdir, 'read_counts.csv'), index=False)
    for chrom in raw:
        os.makedirs(os.path.join(outdir, chrom), exist_ok=True)
        with open(os.path.join(outdir, chrom, 'coverage_matrices_{0}.pkl'.format(chrom)), 'wb') as f:
            pickle.dump(raw[chrom], f)
        with open(os.path.join(outdir, chrom, 'estimated_coverage_matrices_{0}.pkl'.format(chrom)), 'wb') as f:
            pickle.dump(est[chrom], f)
    return outdir


def _matrices(rng, p, length):
    raw = rng.negative_binomial(400, 0.8, size=(p, length)).astype(np.float64)
    est = raw * rng.uniform(0.5, 1.5, size=(p, 1)) * rng.uniform(0.97, 1.03, size=(p, length)) + rng.uniform(0, 1e-4, size=(p, length))
    return raw, est


def write_reference_dir(outdir, seed=11):
    rng = np.random.default_rng(seed)
    rows = [('chr1', 323892, 324060, 'GENE_1'), ('chr1', 324288, 324345, 'GENE_1'),
            ('chr1', 1152288, 1153838, 'GENE_2'), ('chr1', 1153068, 1154013, 'GENE_2')]
    raw, est = {'chr1': {}}, {'chr1': {}}
    for gene, length in (('GENE_1', 225), ('GENE_2', 2495)):
        raw['chr1'][gene], est['chr1'][gene] = _matrices(rng, 2, length)
    return _write(outdir, rows, REFERENCE_SAMPLES, raw, est)


def write_hard_dir(outdir, seed=12):
    rng = np.random.default_rng(seed)
    rows = [('chr1', 100, 400, 'abc1'), ('chr1', 500, 700, 'abc1'), ('chr1', 5000, 5300, 'Def2'), ('chr2', 100, 230, 'ghi3'),
            ('chr2', 900, 1200, 'only_raw'), ('chr2', 3000, 3064, 'jkl4')]
    raw, est = {'chr1': {}, 'chr2': {}}, {'chr1': {}, 'chr2': {}}
    for chrom, gene, length in (('chr1', 'abc1', 500), ('chr1', 'Def2', 300), ('chr2', 'ghi3', 130), ('chr2', 'only_raw', 300),
                                ('chr2', 'jkl4', 64)):
        raw[chrom][gene], est[chrom][gene] = _matrices(rng, 3, length)
    del est['chr2']['only_raw']
    return _write(outdir, rows, HARD_SAMPLES, raw, est)


def write_nan_dir(outdir, seed=13):
    rng = np.random.default_rng(seed)
    rows = [('chr1', 100, 300, 'A1'), ('chr1', 1000, 1150, 'B2'), ('chr1', 2000, 2090, 'C3')]
    raw, est = {'chr1': {}}, {'chr1': {}}
    for gene, length in (('A1', 200), ('B2', 150), ('C3', 90)):
        raw['chr1'][gene], est['chr1'][gene] = _matrices(rng, 2, length)
    est['chr1']['B2'][1, 40] = np.nan
    est['chr1']['B2'][0, 41] = np.nan
    raw['chr1']['B2'][0, 0] = np.inf
    return _write(outdir, rows, REFERENCE_SAMPLES, raw, est)


def tree(root):
    """{relative path: bytes} of every file under root."""
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), 'rb') as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out
