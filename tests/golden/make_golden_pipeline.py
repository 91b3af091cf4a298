"""
Fixtures and goldens of the annotation stage and of the BAM + GTF pipeline, from the real reference.

    python tests/golden/make_golden_pipeline.py /path/to/DegNorm            writes the files below
    python tests/golden/make_golden_pipeline.py /path/to/DegNorm --time     times the reference on the seeded GTF of
                                                                            tools/gtf_speed.py (no file is written)

The reference's modules import pysam and HTSeq only to open BAM files and to find gene overlaps; stub modules stand in for
them, `np.float_` is restored as in make_golden.py, the reads come from tests/_gtf_fixtures.py through a replaced
load_chromosome_reads, and the overlap structure comes from degnorm_amd.gene_processing (as in make_golden_reads.py).

    chr1_small.gtf     the reference's own test annotation (data its tests read), copied
    hard.gtf           seeded: every attribute / feature / duplicate / chromosome-name case the scanner has to get right
    pipeline.gtf       the annotation of the end-to-end fixture (tests/_gtf_fixtures.py)
    annotation.npz     the reference's GeneAnnotationLoader.get_data() and GeneAnnotationProcessor.run() tables of the three
                       files, and run() of hard.gtf with chroms=['1', 'X']
    pipeline.npz       the reference's chain on pipeline.gtf and the seeded reads of three samples: per-sample read counts
                       and overlap coverage, merge_read_counts, merge_overlap_gene_coverage, merge_coverage, the re-ordered
                       tables of __main__.py:175-193 and the genes its filter (:219-247) drops in two cases
"""
import os
import pickle
import shutil
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gtf_fixtures as gf                        # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure  # noqa: E402


def write_hard_gtf(path, seed=5):
    """hard.gtf: see the module docstring of tests/test_gpu_annotation.py for what each block is there for."""
    rng = np.random.default_rng(seed)
    L = []

    def line(chrom, feature, a, b, attr, source='src'):
        L.append('{0}\t{1}\t{2}\t{3}\t{4}\t.\t+\t.\t{5}'.format(chrom, source, feature, a, b, attr))

    # gene_name before gene_id, after it, and gene_id alone
    line('1', 'gene', 100, 900, 'gene_id "G1"; gene_name "AB1";')
    line('1', 'exon', 100, 300, 'gene_name "AB1"; gene_id "G1"; transcript_id "T1";')
    line('1', 'exon', 500, 900, 'gene_id "G1"; transcript_id "T1"; gene_name "AB1";')
    line('1', 'transcript', 100, 900, 'gene_id "G1"; transcript_id "T1";')
    line('1', 'CDS', 120, 280, 'gene_id "G1"; gene_name "AB1";')
    line('1', 'Exon', 1500, 1800, 'gene_id "AB10"; transcript_id "T2";')
    line('1', 'EXON', 2000, 2400, 'gene_id "AB10"; transcript_id "T2"')                      # no trailing ';'
    # an empty gene_name falls through to gene_id; blanks around ';'
    line('1', 'exon', 3000, 3300, 'gene_name ""; gene_id "G3";')
    line('1', 'exon', 3400, 3600, '  gene_id   "G3"  ;   transcript_id "T3"  ;  ')
    line('1', 'exon', 3500, 3900, 'transcript_id "T3b" ; gene_id "G3" ;gene_name  "" ;')
    # exact duplicates, duplicates that differ only in the transcript, overlapping exons
    for _ in range(3):
        line('10', 'exon', 700, 1000, 'gene_id "G4"; gene_name "DUP"; transcript_id "T4";')
    line('10', 'exon', 700, 1000, 'gene_id "G4"; gene_name "DUP"; transcript_id "T4b";')
    line('10', 'exon', 900, 1400, 'gene_id "G4"; gene_name "DUP"; transcript_id "T4b";')
    line('10', 'exon', 950, 1200, 'gene_id "G4"; gene_name "DUP"; transcript_id "T4c";')
    # a gene on two chromosomes (vanishes, unless the subset drops one of them first), next to one that stays
    line('X', 'exon', 100, 400, 'gene_id "G5"; gene_name "TWO";')
    line('10', 'exon', 5000, 5400, 'gene_id "G5"; gene_name "TWO";')
    line('X', 'exon', 800, 1200, 'gene_id "G6"; gene_name "ONLYX";')
    line('chrUn_gl000220', 'exon', 10, 500, 'gene_id "G7"; gene_name "UN1";')
    line('chrUn_gl000220', 'gene', 10, 500, 'gene_id "G7"; gene_name "UN1";')
    # seeded genes: random order of the tags, random feature spelling, several chromosomes
    for g in range(40):
        chrom = ['1', '10', 'X', 'chrUn_gl000220'][int(rng.integers(0, 4))]
        base = 10000 + 3000 * g
        name, gid = 'S{0}'.format(g), 'SID{0}'.format(g)
        for e in range(int(rng.integers(1, 5))):
            a = base + 400 * e + int(rng.integers(0, 100))
            b = a + int(rng.integers(50, 600))
            tags = ['gene_id "{0}"'.format(gid), 'transcript_id "T{0}_{1}"'.format(g, int(rng.integers(0, 2))), 'exon_number {0}'.format(e)]
            if g % 3:
                tags.insert(int(rng.integers(0, len(tags) + 1)), 'gene_name "{0}"'.format(name))
            feature = ['exon', 'Exon', 'EXON', 'exon', 'CDS', 'start_codon'][int(rng.integers(0, 6))]
            line(chrom, feature, a, b, '; '.join(tags) + (';' if rng.random() < 0.7 else ''))
    # one line of about 100 KB of attributes, its gene_name at the very end
    filler = '; '.join('note_{0} "{1}"'.format(k, 'x' * 40) for k in range(2000))
    line('X', 'exon', 200000, 200900, 'gene_id "GBIG"; ' + filler + '; gene_name "BIG";')
    line('X', 'exon', 201000, 201500, 'gene_id "GBIG"; gene_name "BIG";')
    # the last line has no newline
    with open(path, 'w') as f:
        f.write('\n'.join(L))
    return len(L)


def frame_arrays(out, key, df):
    for c in df.columns:
        v = df[c].values
        out['{0}_{1}'.format(key, c)] = v.astype(str) if v.dtype == object else v.astype(np.int64)
    out[key + '_index'] = np.asarray(df.index, dtype=np.int64)


def annotation_goldens(GeneAnnotationLoader, GeneAnnotationProcessor):
    out = {}
    for name in ('chr1_small', 'hard', 'pipeline'):
        path = os.path.join(HERE, name + '.gtf')
        frame_arrays(out, name + '_data', GeneAnnotationLoader(path).get_data())
        run = GeneAnnotationProcessor(path, verbose=False).run()
        frame_arrays(out, name + '_run', run)
        print(name, 'get_data', out[name + '_data_start'].size, 'rows; run', len(run), 'rows,', run.gene.nunique(), 'genes')
    sub = GeneAnnotationProcessor(os.path.join(HERE, 'hard.gtf'), chroms=['1', 'X'], verbose=False).run()
    assert 'TWO' in set(sub.gene) and 'TWO' not in set(out['hard_run_gene'].tolist())
    frame_arrays(out, 'hard_sub_run', sub)
    np.savez_compressed(os.path.join(HERE, 'annotation.npz'), **out)


def pipeline_goldens(R, M, GeneAnnotationProcessor):
    import pandas as pd
    out = {}
    gtf = os.path.join(HERE, 'pipeline.gtf')
    chroms = [name for name, _ in gf.PIPELINE_REFS]                                   # every sample has the same header
    chroms = np.intersect1d(chroms, chroms).tolist()
    exon_df = GeneAnnotationProcessor(gtf, verbose=False, chroms=chroms).run()
    chroms = np.intersect1d(chroms, exon_df.chr.unique()).tolist()
    exon_df = exon_df[exon_df.chr.isin(chroms)]
    genes_df = exon_df[['chr', 'gene', 'gene_start', 'gene_end']].drop_duplicates().reset_index(drop=True)
    overlap = {c: get_gene_overlap_structure(genes_df[genes_df.chr == c]) for c in chroms}
    work = tempfile.mkdtemp(prefix='dn_pipeline_')
    try:
        for k, s in enumerate(gf.PIPELINE_SAMPLES):
            reads = gf.pipeline_reads(k)
            p = R.BamReadsProcessor.__new__(R.BamReadsProcessor)
            p.header = pd.DataFrame(gf.PIPELINE_REFS, columns=['chr', 'length'])
            p.paired, p.sample_id, p.save_dir, p.verbose, p.n_jobs, p.chroms = False, s, os.path.join(work, s), False, 1, chroms
            p.load_chromosome_reads = lambda c, reads=reads: reads[c].copy()
            p.coverage_read_counts(overlap, gene_df=genes_df, exon_df=exon_df)
            for c in chroms:                                                        # the per-sample files, for the host tests
                cnt = pd.read_csv(os.path.join(work, s, 'read_counts_{0}_{1}.csv'.format(s, c)))
                out['counts_{0}_genes'.format(c)] = cnt.gene.values.astype(str)
                out['counts_{0}_{1}'.format(c, s)] = cnt[s].values.astype(np.int64)
                f_ol = os.path.join(work, s, 'overlap_coverage_{0}_{1}.pkl'.format(s, c))
                with open(f_ol, 'rb') as f:
                    ol = pickle.load(f)
                out['ol_{0}_genes'.format(c)] = np.array(list(ol.keys()))
                out['ol_{0}_len'.format(c)] = np.array([ol[g].size for g in ol], dtype=np.int64)
                out['ol_{0}_{1}'.format(c, s)] = np.concatenate([ol[g] for g in ol]).astype(np.int64)
                out['has_csr_{0}_{1}'.format(c, s)] = np.int32(os.path.isfile(os.path.join(work, s, 'chrom_coverage_{0}_{1}.npz'.format(s, c))))
        sample_ids = list(gf.PIPELINE_SAMPLES)
        read_count_df = M.merge_read_counts(work, sample_ids=sample_ids, chroms=chroms)
        frame_arrays(out, 'merged_counts', read_count_df)
        for c in chroms:
            mo = M.merge_overlap_gene_coverage(work, sample_ids, c)
            out['merged_ol_{0}_genes'.format(c)] = np.array(list(mo.keys()))
            out['merged_ol_{0}_len'.format(c)] = np.array([mo[g].shape[1] for g in mo], dtype=np.int64)
            out['merged_ol_{0}_flat'.format(c)] = np.concatenate([mo[g].reshape(-1) for g in mo]) if mo else np.zeros(0)
        gene_cov_dict = M.merge_coverage(work, sample_ids=sample_ids, exon_df=exon_df, n_jobs=1, output_dir=work, verbose=False)
        for c in chroms:
            with open(os.path.join(work, c, 'coverage_matrices_{0}.pkl'.format(c)), 'rb') as f:
                out['pkl_{0}_genes'.format(c)] = np.array(list(pickle.load(f).keys()))
    finally:
        shutil.rmtree(work)
    genes = list(gene_cov_dict.keys())
    genes_df = genes_df.set_index('gene').loc[genes].reset_index(drop=False)            # __main__.py:179-193
    read_count_df = read_count_df.set_index('gene').loc[genes].reset_index(drop=False)
    exon_df = exon_df[exon_df.gene.isin(genes)]
    frame_arrays(out, 'exon', exon_df)
    frame_arrays(out, 'genes', genes_df)
    frame_arrays(out, 'read_counts', read_count_df)
    out['chroms'] = np.array(chroms)
    out['sample_ids'] = np.array(sample_ids)
    out['cov_genes'] = np.array(genes)
    out['cov_len'] = np.array([gene_cov_dict[g].shape[1] for g in genes], dtype=np.int64)
    out['cov_flat'] = np.concatenate([gene_cov_dict[g].reshape(-1) for g in genes])
    assert all(gene_cov_dict[g].dtype == np.float64 for g in genes)

    def dropped(minimax_coverage, downsample_rate):                                  # __main__.py:219-231
        return [g for g in genes_df.gene if gene_cov_dict[g].max() < minimax_coverage or gene_cov_dict[g].shape[1] <= downsample_rate]

    peaks = sorted(gene_cov_dict[g].max() for g in genes)
    case_a = int(peaks[0]) + 1
    assert peaks[0] < case_a <= peaks[1]
    case_b = int(min(out['cov_len']))
    drop_a, drop_b = dropped(case_a, 1), dropped(0, case_b)
    assert len(drop_a) >= 1 and len(genes) - len(drop_a) >= 6
    assert len(drop_b) >= 1 and len(genes) - len(drop_b) >= 2
    out['case_a_minimax'], out['case_a_dropped'] = np.int64(case_a), np.array(drop_a)
    out['case_b_downsample'], out['case_b_dropped'] = np.int64(case_b), np.array(drop_b)
    np.savez_compressed(os.path.join(HERE, 'pipeline.npz'), **out)
    print('pipeline:', ' '.join(genes), '| A: minimax', case_a, 'drops', drop_a, '| B: rate', case_b, 'drops', drop_b)


def time_reference(GeneAnnotationProcessor, min_bytes):
    d = tempfile.mkdtemp(prefix='dn_gtf_time_')
    try:
        path = os.path.join(d, 'seeded.gtf')
        n_lines, n_genes, size = gf.write_gtf(path, 7, min_bytes, header=False)          # the reference refuses `#` lines
        t0 = time.perf_counter()
        df = GeneAnnotationProcessor(path, verbose=False).run()
        print('reference GeneAnnotationProcessor.run on this host: {0:.1f} s for {1} bytes, {2} lines, {3} genes -> {4} rows'
              .format(time.perf_counter() - t0, size, n_lines, n_genes, len(df)))
    finally:
        shutil.rmtree(d)


def main(ref_root, timing=False):
    for stub in ('pysam', 'HTSeq'):
        sys.modules.setdefault(stub, types.ModuleType(stub))
    if not hasattr(np, 'float_'):
        np.float_ = np.float64
    sys.path.insert(0, ref_root)
    from degnorm import reads as R
    from degnorm import reads_coverage_merge as M
    from degnorm.loaders import GeneAnnotationLoader
    from degnorm.gene_processing import GeneAnnotationProcessor
    if timing:
        time_reference(GeneAnnotationProcessor, int(os.environ.get('GTF_BYTES', 1500 << 20)))
        return
    shutil.copyfile(os.path.join(ref_root, 'degnorm', 'tests', 'data', 'chr1_small.gtf'), os.path.join(HERE, 'chr1_small.gtf'))
    print('hard.gtf:', write_hard_gtf(os.path.join(HERE, 'hard.gtf')), 'lines')
    gf.write_pipeline_gtf(os.path.join(HERE, 'pipeline.gtf'))
    annotation_goldens(GeneAnnotationLoader, GeneAnnotationProcessor)
    pipeline_goldens(R, M, GeneAnnotationProcessor)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--time']
    main(args[0] if args else os.environ.get('DEGNORM_REF', '../DegNorm'), timing='--time' in sys.argv)
