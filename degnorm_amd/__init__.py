"""
degnorm_amd -- MI355X-native NMF over-approximation core of DegNorm (hot path only).

    from degnorm_amd import GeneNMFOA            # mirror of degnorm.nmf.GeneNMFOA (reference nmf.py:10)
    from degnorm_amd import run_gene_nmfoa_mpi   # mirror of degnorm.nmf_mpi.run_gene_nmfoa_mpi (nmf_mpi.py:555)
    from degnorm_amd import GeneAnnotationLoader, GeneAnnotationProcessor      # .gtf -> exon table (device GTF scan)
    from degnorm_amd import run_pipeline, prepare_inputs                        # .bam + .gtf -> results (python -m degnorm_amd)
"""
__version__ = '0.1.0'


def __getattr__(name):
    # lazy: importing the package (e.g. for degnorm_amd.synth) must not need the HIP library.
    if name in ('GeneNMFOA',):
        from . import nmf
        return getattr(nmf, name)
    if name in ('run_gene_nmfoa_mpi', 'save_results'):
        from . import nmf_mpi
        return getattr(nmf_mpi, name)
    if name == 'GeneAnnotationLoader':
        from . import loaders
        return loaders.GeneAnnotationLoader
    if name in ('GeneAnnotationProcessor', 'get_gene_overlap_structure'):
        from . import gene_processing
        return getattr(gene_processing, name)
    if name in ('merge_read_counts', 'merge_overlap_gene_coverage', 'merge_coverage', 'merge_chrom_coverage'):
        from . import coverage_merge
        return getattr(coverage_merge, name)
    if name in ('run_pipeline', 'prepare_inputs'):
        from . import pipeline
        return getattr(pipeline, name)
    raise AttributeError(name)
