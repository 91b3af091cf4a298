"""
DegNorm end to end from .bam and .gtf or .gff3 files (reference: `degnorm/__main__.py:56-286`).

    prepare_inputs(bam_files, bai_files, genome_annotation, output_dir, ...)   everything up to the NMF-OA input
    run_pipeline(bam_files, bai_files, genome_annotation, output_dir, ...)     prepare_inputs, GeneNMFOA.run, save_results

Every stage is the library's own: NativeBamReadsProcessor reads the alignments (no pysam), GeneAnnotationProcessor the
annotation (device GTF or GFF3 scan), merge_coverage assembles the gene matrices on the device.  The output directory ends up as
the reference leaves it -- gene_exon_metadata.csv, read_counts.csv, <chr>/coverage_matrices_<chr>.pkl and the result
files -- so warm_start.load_from_previous and `python -m degnorm_amd -w` accept it.
"""
import logging
import os
import shutil

import numpy as np

from .bam import NativeBamReadsProcessor, check_read_options, check_stranded
from .coverage_merge import merge_coverage, merge_read_counts
from .gene_processing import GeneAnnotationProcessor, get_gene_overlap_structure
from .utils import subset_to_chrom
from .warm_start import select_genes


def prepare_inputs(bam_files, bai_files, genome_annotation, output_dir, downsample_rate=1, minimax_coverage=0,
                   unique_alignment=True, n_jobs=1, verbose=True, device=None, inflate='host', frame='host', verify=False,
                   pair='host', pairing='name', exclude_flags=0, require_flags=0, min_mapq=0, stranded='no'):
    """
    The reference's .bam preprocessing path and gene filter (__main__.py:56-247): chromosomes common to every .bam header and
    the annotation, per-sample coverage and read counts, their merge (coverage matrices pickled per chromosome into
    output_dir, per-sample directories removed), the gene tables re-ordered to the coverage dict, gene_exon_metadata.csv and
    read_counts.csv, then the filter on maximum coverage and length.  inflate, frame: NativeBamReadsProcessor's
    (each 'host' or 'device'); verify: check every BGZF block read against the CRC32 of its trailer; pair: where the mates of
    paired-end files are paired ('host': the reference's order; 'device': on the GPU, equal names in file order).  pairing
    ('name', 'flag' or 'auto'), exclude_flags, require_flags, min_mapq: which records form a fragment and which are dropped
    first (NativeBamReadsProcessor); a bad value is a ValueError before any file is opened.  stranded ('no', 'forward' or
    'reverse'; include/degnorm_amd.h, "Strand-specific counting"): count reads by strand -- the annotation keeps its strand
    column, genes without a single strand are left out, every chromosome is counted per strand, the tables and
    gene_exon_metadata.csv carry `strand`, and the genes of a chromosome come '+' first, then '-'.

    :return: (gene_cov_dict, read_count_df, genes_df, exon_df, sample_ids)
    """
    check_read_options(pairing, exclude_flags, require_flags, min_mapq)
    by_strand = check_stranded(stranded) != 'no'
    chroms = list()
    for bam_file, bai_file in zip(bam_files, bai_files):
        header = NativeBamReadsProcessor(bam_file, index_file=bai_file, verbose=False, verify=verify).header
        new_chroms = header.chr.values.tolist()
        chroms = new_chroms if not chroms else np.intersect1d(chroms, new_chroms).tolist()

    logging.info('Begin genome annotation file processing...')
    exon_df = GeneAnnotationProcessor(genome_annotation, verbose=verbose, chroms=chroms, **({'strand': True} if by_strand else {})).run()
    chroms = np.intersect1d(chroms, exon_df.chr.unique()).tolist()
    exon_df = exon_df[exon_df.chr.isin(chroms)]
    genes_df = exon_df[['chr', 'gene', 'gene_start', 'gene_end'] + (['strand'] if by_strand else [])].drop_duplicates().reset_index(drop=True)
    logging.info('Found {0} chromosomes in intersection of all experiments and gene annotation data:\n'
                 '\t{1}'.format(len(chroms), ', '.join(chroms)))

    gene_overlap_dict = {chrom: get_gene_overlap_structure(subset_to_chrom(genes_df, chrom=chrom)) for chrom in chroms}
    # a stranded run counts each strand's genes with their own structure (the reader builds it again per chromosome): so is the rate
    counted = [get_gene_overlap_structure(subset_to_chrom(genes_df[genes_df['strand'] == s], chrom=chrom)) for chrom in chroms
               for s in ('+', '-')] if by_strand else list(gene_overlap_dict.values())
    n_overlap = sum(len(g) for d in counted for g in d['overlap_genes'])
    n_isolated = sum(len(d['isolated_genes']) for d in counted)
    logging.info('Rate of gene overlap: {0} / {1}'.format(n_overlap, n_isolated + n_overlap))

    sample_ids = list()
    for idx, (bam_file, bai_file) in enumerate(zip(bam_files, bai_files)):
        logging.info('Loading RNA-seq data file {0} / {1}'.format(idx + 1, len(bam_files)))
        reader = NativeBamReadsProcessor(bam_file, index_file=bai_file, chroms=chroms, n_jobs=n_jobs, output_dir=output_dir,
                                         unique_alignment=unique_alignment, verbose=verbose, inflate=inflate, frame=frame,
                                         verify=verify, pair=pair, pairing=pairing, exclude_flags=exclude_flags,
                                         require_flags=require_flags, min_mapq=min_mapq, **({'stranded': stranded} if by_strand else {}))
        sample_ids.append(reader.sample_id)
        reader.coverage_read_counts(gene_overlap_dict, gene_df=genes_df, exon_df=exon_df)

    logging.info('Merging read counts across samples.')
    read_count_df = merge_read_counts(output_dir, sample_ids=sample_ids, chroms=chroms)
    logging.info('Merging gene coverage arrays across samples and saving results to chromosome directories.')
    gene_cov_dict = merge_coverage(output_dir, sample_ids=sample_ids, exon_df=exon_df, n_jobs=n_jobs, output_dir=output_dir,
                                   verbose=verbose, device=device)
    for s_id in sample_ids:
        shutil.rmtree(os.path.join(output_dir, s_id))

    # gene tables in the coverage dict's order; only the exons of its genes (__main__.py:175-193)
    genes = list(gene_cov_dict.keys())
    genes_df = genes_df.set_index('gene').loc[genes].reset_index(drop=False)
    read_count_df = read_count_df.set_index('gene').loc[genes].reset_index(drop=False)
    exon_df = exon_df[exon_df.gene.isin(genes)]
    if genes_df.shape[0] != read_count_df.shape[0]:
        raise ValueError('Genes DataFrame and read counts DataFrame do not have same number of rows!')
    exon_df.to_csv(os.path.join(output_dir, 'gene_exon_metadata.csv'), index=False)
    read_count_df.to_csv(os.path.join(output_dir, 'read_counts.csv'), index=False)

    logging.info('Determining genes to include in DegNorm coverage curve approximation.')
    gene_cov_dict, read_count_df, genes_df = select_genes(gene_cov_dict, read_count_df, genes_df,
                                                          minimax_coverage=minimax_coverage, downsample_rate=downsample_rate)
    return gene_cov_dict, read_count_df, genes_df, exon_df, sample_ids


def run_pipeline(bam_files, bai_files, genome_annotation, output_dir, degnorm_iter=5, nmf_iter=100, downsample_rate=1,
                 minimax_coverage=0, skip_baseline_selection=False, unique_alignment=True, n_jobs=1, verbose=True, device=None,
                 inflate='host', frame='host', verify=False, pair='host', pairing='name', exclude_flags=0, require_flags=0, min_mapq=0,
                 stranded='no'):
    """
    DegNorm on .bam files and a .gtf or .gff3 annotation, results written to output_dir (an existing directory).  verify: check every
    BGZF block read against the CRC32 of its trailer (ValueError naming the file and the block).  pairing, exclude_flags,
    require_flags, min_mapq, stranded: as for prepare_inputs.

    :return: (fitted GeneNMFOA, estimates, gene_cov_dict, read_count_df, genes_df, exon_df, sample_ids)
    """
    from .nmf import GeneNMFOA
    gene_cov_dict, read_count_df, genes_df, exon_df, sample_ids = prepare_inputs(
        bam_files, bai_files, genome_annotation, output_dir, downsample_rate=downsample_rate, minimax_coverage=minimax_coverage,
        unique_alignment=unique_alignment, n_jobs=n_jobs, verbose=verbose, device=device, inflate=inflate, frame=frame,
        verify=verify, pair=pair, pairing=pairing, exclude_flags=exclude_flags, require_flags=require_flags, min_mapq=min_mapq,
        stranded=stranded)
    logging.info('RNA-seq sample identifiers: \n\t' + ', '.join(sample_ids))
    logging.info('DegNorm will run on {0} genes, downsampling rate = 1 / {1}, {2} baseline selection.'
                 .format(len(gene_cov_dict), downsample_rate, 'without' if skip_baseline_selection else 'with'))
    nmfoa = GeneNMFOA(degnorm_iter=degnorm_iter, nmf_iter=nmf_iter, downsample_rate=downsample_rate, n_jobs=n_jobs,
                      skip_baseline_selection=skip_baseline_selection, device=device)
    estimates = nmfoa.run(gene_cov_dict, reads_dat=read_count_df[sample_ids].values.astype(np.float64))
    nmfoa.save_results(estimates, gene_manifest_df=genes_df, output_dir=output_dir, sample_ids=sample_ids)
    return nmfoa, estimates, gene_cov_dict, read_count_df, genes_df, exon_df, sample_ids
