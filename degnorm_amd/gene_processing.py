"""
Gene overlap structure of one chromosome (reference: `degnorm/gene_processing.py:126-231`).

The reference builds an HTSeq GenomicArrayOfSets of the gene spans, a dense n x n adjacency matrix and walks it with
networkx; neither HTSeq nor `nx.from_numpy_matrix` (removed in networkx 3.4) is available on this stack.  Two genes
overlap when their 0-based half-open spans [gene_start - 1, gene_end) intersect -- the test the reference's
GenomicArrayOfSets query makes -- so genes whose spans merely touch (one ends at base b, the next starts at b + 1) do not
overlap.  The groups are the connected components of that relation, which one sort-and-sweep over the spans finds in
O(n log n).
"""
import numpy as np


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
