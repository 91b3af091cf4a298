"""
Annotation processing (reference: `degnorm/gene_processing.py`): GeneAnnotationProcessor (:8-123) turns a .gtf or .gff3 file into
the exon table the reads stage, the coverage merge and the result writer take, and get_gene_overlap_structure (:126-231)
splits one chromosome's genes into overlap groups and isolated genes.

GeneAnnotationProcessor loads the file through the device scanner (loaders.py); the table work after it is grouped
pandas / numpy on integer codes: no Python call per gene (the reference's gene_outline runs a lambda per gene).

For the overlap structure the reference builds an HTSeq GenomicArrayOfSets of the gene spans, a dense n x n adjacency matrix and walks it with
networkx; neither HTSeq nor `nx.from_numpy_matrix` (removed in networkx 3.4) is available on this stack.  Two genes
overlap when their 0-based half-open spans [gene_start - 1, gene_end) intersect -- the test the reference's
GenomicArrayOfSets query makes -- so genes whose spans merely touch (one ends at base b, the next starts at b + 1) do not
overlap.  The groups are the connected components of that relation, which one sort-and-sweep over the spans finds in
O(n log n).
"""
import logging

import numpy as np

from .loaders import annotation_loader
from .utils import subset_to_chrom


class GeneAnnotationProcessor(object):

    def __init__(self, annotation_file, chroms=None, verbose=True, strand=False):
        """
        :param annotation_file: str .gtf, .gff3 or .gff file
        :param chroms: str or list of str chromosome names: subset the annotation to them
        :param verbose: bool write progress to the logger?
        :param strand: bool strand-specific counting (include/degnorm_amd.h): keep the `strand` column of the exon lines.  A
        gene is on '+' or '-' when all its exon rows say so; a gene with '.', '?' or both strands among its rows is unstranded
        and is left out, with one warning that gives their number and up to ten names; self.unstranded_genes keeps them all.
        """
        self.strand = bool(strand)
        self.unstranded_genes = []
        self.filename = annotation_file
        self.verbose = verbose
        self.chroms = chroms
        self.loader = None
        if self.chroms:
            if not isinstance(self.chroms, list):
                self.chroms = [self.chroms]

    def load(self):
        """The exon rows of the file (the get_data of the loader its extension picks), subset to self.chroms when given."""
        self.loader = annotation_loader(self.filename)
        return self._subset(self.loader.get_data(strand=True) if self.strand else self.loader.get_data())

    def _subset(self, exon_df):
        if self.chroms:
            if self.verbose:
                logging.info('Subsetting exon data to {0} chromosomes:\n'
                             '\t{1}'.format(len(self.chroms), ', '.join(self.chroms)))
            exon_df = subset_to_chrom(exon_df, chrom=self.chroms)
        if self.verbose:
            logging.info('Successfully loaded exon data -- shape: {0}'.format(exon_df.shape))
        if exon_df.empty:
            raise ValueError('Exon DataFrame is empty!')
        return exon_df

    @staticmethod
    def remove_multichrom_genes(df):
        """df without the genes that show up on more than one chromosome."""
        per_gene = df.groupby('gene').chr.nunique()
        return df[~df.gene.isin(per_gene[per_gene > 1].index.tolist())]

    @staticmethod
    def gene_outline(df):
        """
        min(start) and max(end) of every (chr, gene) of an exon table: DataFrame of `chr`, `gene`, `gene_start`, `gene_end`,
        sorted by chr, then gene (as the reference's groupby).
        """
        grp = df.groupby(['chr', 'gene'])
        return grp.agg(gene_start=('start', 'min'), gene_end=('end', 'max')).reset_index()

    def process(self, exon_df):
        """The steps of run() after load(): multi-chromosome genes out, gene outlines joined on, duplicates dropped."""
        exon_df = self.remove_multichrom_genes(exon_df).drop_duplicates()
        if self.strand:
            exon_df = self.stranded_genes(exon_df)
        gene_df = self.gene_outline(exon_df)
        exon_df = exon_df.merge(gene_df, on=['chr', 'gene']).drop_duplicates()
        return exon_df

    def stranded_genes(self, exon_df):
        """The exon rows of the genes whose rows all say '+' or all say '-'; the other genes go to self.unstranded_genes."""
        per_gene = exon_df.groupby('gene', sort=False)['strand'].agg(['first', 'nunique'])
        ok = (per_gene['nunique'] == 1) & per_gene['first'].isin(['+', '-'])
        self.unstranded_genes = per_gene.index[~ok.values].tolist()
        if self.unstranded_genes:
            logging.warning('{0} genes without a single strand (., ? or both strands among their exon lines) are left out of the '
                            'stranded run: {1}{2}'.format(len(self.unstranded_genes), ', '.join(self.unstranded_genes[:10]),
                                                          ', ...' if len(self.unstranded_genes) > 10 else ''))
        if exon_df.empty:
            return exon_df
        return exon_df[exon_df['gene'].isin(per_gene.index[ok.values])]

    def run(self):
        """
        Load the annotation file, remove the genes that occur on several chromosomes, outline every gene and drop
        duplicates (reference gene_processing.py:89-123).

        :return: DataFrame with `chr`, `start`, `end`, `gene`, `gene_start`, `gene_end`: the exons, in file order; with
        strand=True also `strand`, '+' or '-', the strand of the row's gene.
        """
        if self.verbose:
            logging.info('Loading genome annotation file {0}...'.format(self.filename))
        exon_df = self.load()
        if self.verbose:
            logging.info('Begin genome annotation file processing.')
        exon_df = self.process(exon_df)
        if self.verbose:
            logging.info('Processing successful. Final shape -- {0}'.format(exon_df.shape))
        return exon_df


def get_gene_overlap_structure(gene_df):
    """
    Split a chromosome's genes into groups of mutually reachable overlapping genes and isolated genes.

    :param gene_df: pandas.DataFrame with `gene`, `gene_start`, `gene_end` columns (1-based, inclusive ends).
    :return: {'overlap_genes': list of lists of gene names, 'isolated_genes': list of gene names} -- the same partition
    and the same isolated set as the reference.  Order: groups by their first gene in gene_df order, genes within a
    group in gene_df order, isolated genes in gene_df order (the reference orders groups by networkx's search, which
    this does not try to reproduce).
    """
    genes = gene_df['gene'].values
    n = len(genes)
    if n == 0:
        return {'overlap_genes': [], 'isolated_genes': []}
    lo = gene_df['gene_start'].values.astype(np.int64) - 1
    hi = gene_df['gene_end'].values.astype(np.int64)
    order = np.argsort(lo, kind='stable')
    comp = np.empty(n, dtype=np.int64)
    c, reach = -1, None
    for i in order.tolist():
        if reach is None or lo[i] >= reach:        # half-open spans: a start at the running end does not intersect
            c += 1
            reach = hi[i]
        else:
            reach = max(reach, hi[i])
        comp[i] = c
    members = {}
    for i in range(n):                              # gene_df order, so groups come out keyed by their first gene
        members.setdefault(int(comp[i]), []).append(i)
    overlap_genes, isolated_genes = [], []
    for idx in members.values():
        if len(idx) == 1:
            isolated_genes.append(genes[idx[0]])
        else:
            overlap_genes.append(genes[idx].tolist())
    return {'overlap_genes': overlap_genes, 'isolated_genes': isolated_genes}
