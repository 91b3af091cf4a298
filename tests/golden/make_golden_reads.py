"""
Goldens of the reads -> coverage / read counts path (tests/golden/reads.npz, tests/golden/reads_edges.npz) from the real
reference.

    python tests/golden/make_golden_reads.py /path/to/DegNorm

The reference's degnorm.reads imports pysam only to open BAM files; a stub module stands in for it, the reads come from
tests/_reads_fixtures.py through a replaced load_chromosome_reads, and header / paired / sample_id are set by hand.  The
overlap structure comes from degnorm_amd.gene_processing (the reference's needs HTSeq).  Cases:
  se   single-end reads on the golden layout (overlap groups, nested exons, touching isolated genes, a gene without reads)
  pe   paired reads on the same layout (overlapping / contained / spliced mates, swapped mate order, orphans)
  qi   single-end reads on a chromosome whose isolated stage gets no read (no chrom_coverage file)
  fz   random CIGAR strings and the reference's cigar_segment_bounds output (nseg 0: ValueError)

reads_edges.npz holds the seeded edge cases of _reads_fixtures.edge_case (random annotations, the groups-only and the
isolated-only variant, every read mutator) and the two segment-cap cases (_reads_fixtures.cap_reads: DN_READS_MAX_SEG M ops
per row) under the keys e00, e01, ... in the same layout, each with the census of
tests/_reads_oracle.py (<key>_census, in the order of census_keys).  Units with a bound below 0 -- which the library drops
and the reference does not -- are taken out of these cases first, found by the restatement; and the restatement has to
reproduce the reference's outputs here, or the script stops.
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_fixtures as rf                      # noqa: E402
import _reads_oracle as ro                        # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure  # noqa: E402


def pack(out, key, reads_df, paired, layout, ref_outputs):
    chrom, chrom_len, genes = layout
    gene_df, exon_df = rf.tables(chrom, genes)
    ov = get_gene_overlap_structure(gene_df)
    enc = [c.encode() for c in reads_df.cigar]
    out[key + '_pos'] = reads_df.pos.values.astype(np.int64)
    out[key + '_cig'] = np.frombuffer(b''.join(enc), dtype=np.uint8)
    out[key + '_cig_off'] = np.r_[0, np.cumsum([len(e) for e in enc])].astype(np.int64)
    if paired:
        out[key + '_pair'] = np.array([int(q[1:]) for q in reads_df.qname_unpaired], dtype=np.int32)
    out[key + '_chrom_len'] = np.int64(chrom_len)
    out[key + '_gene'] = gene_df.gene.values.astype('U8')
    out[key + '_gene_start'] = gene_df.gene_start.values.astype(np.int64)
    out[key + '_gene_end'] = gene_df.gene_end.values.astype(np.int64)
    out[key + '_exon_gene'] = exon_df.gene.values.astype('U8')
    out[key + '_exon_start'] = exon_df.start.values.astype(np.int64)
    out[key + '_exon_end'] = exon_df.end.values.astype(np.int64)
    grp = np.full(len(gene_df), -1, dtype=np.int32)
    for k, g in enumerate(ov['overlap_genes']):
        grp[gene_df.gene.isin(g).values] = k
    out[key + '_group'] = grp
    csr, ol, counts = ref_outputs
    out[key + '_has_csr'] = np.int32(csr is not None)
    out[key + '_csr_idx'] = csr.indices.astype(np.int32) if csr is not None else np.zeros(0, np.int32)
    out[key + '_csr_val'] = csr.data.astype(np.int64) if csr is not None else np.zeros(0, np.int64)
    names = list(ol.keys())
    out[key + '_ol_gene'] = np.array(names, dtype='U8')
    out[key + '_ol_off'] = np.r_[0, np.cumsum([ol[g].size for g in names])].astype(np.int64)
    out[key + '_ol_cov'] = np.concatenate([ol[g] for g in names]).astype(np.int64) if names else np.zeros(0, np.int64)
    out[key + '_counts'] = np.array([counts[g] for g in gene_df.gene], dtype=np.int64)


def run_reference(R, reads_df, paired, layout, workdir):
    import pandas as pd
    from scipy import sparse
    chrom, chrom_len, genes = layout
    gene_df, exon_df = rf.tables(chrom, genes)
    ov = get_gene_overlap_structure(gene_df)
    p = R.BamReadsProcessor.__new__(R.BamReadsProcessor)
    p.header = pd.DataFrame({'chr': [chrom], 'length': [chrom_len]})
    p.paired, p.sample_id, p.save_dir, p.verbose = paired, 's1', workdir, False
    p.load_chromosome_reads = lambda c: reads_df.copy()
    p.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
    f_csr = os.path.join(workdir, 'chrom_coverage_s1_{0}.npz'.format(chrom))
    csr = sparse.load_npz(f_csr) if os.path.isfile(f_csr) else None
    f_ol = os.path.join(workdir, 'overlap_coverage_s1_{0}.pkl'.format(chrom))
    ol = {}                                       # no overlap group: the reference writes no file
    if os.path.isfile(f_ol):
        with open(f_ol, 'rb') as f:
            ol = pickle.load(f)
    cnt = pd.read_csv(os.path.join(workdir, 'read_counts_s1_{0}.csv'.format(chrom)))
    return csr, ol, dict(zip(cnt.gene, cnt.s1))


# (layout seed, paired, variant) of the cases e00, e01, ...; the segment-cap cases follow them
EDGE_CASES = [(s, p, None) for s in range(5) for p in (False, True)] + \
             [(5, p, v) for v in ('groups_only', 'isolated_only') for p in (False, True)]


def without_negative_units(df, layout, paired):
    """The case without the units the library drops for a bound below 0, and its census (negative_bound == 0)."""
    chrom, chrom_len, genes = layout
    gene_df, exon_df = rf.tables(chrom, genes)
    ov = get_gene_overlap_structure(gene_df)
    while True:
        trace = {}
        res = ro.restate(df, chrom_len, ov, gene_df, exon_df, paired, trace=trace)
        if not trace['negative_rows']:
            assert res[3]['negative_bound'] == 0
            return df, res
        df = df.drop(df.index[trace['negative_rows']]).reset_index(drop=True)


def edge_cases(R):
    out, total = {'census_keys': np.array(ro.CENSUS_KEYS, dtype='U32')}, []
    cases = [rf.edge_case(seed, paired, variant=variant) + (paired, 'seed {0} {1}'.format(seed, variant or '')) for seed, paired, variant in EDGE_CASES]
    cases += [(rf.cap_reads(paired, rf.reads_max_seg()), rf.cap_layout(), paired, 'segment cap') for paired in (False, True)]
    for k, (df, layout, paired, what) in enumerate(cases):
        key = 'e{0:02d}'.format(k)
        df, restated = without_negative_units(df, layout, paired)
        with tempfile.TemporaryDirectory() as d:
            res = run_reference(R, df, paired, layout, d)
        ro.assert_same((res[0], {g: v.astype(np.int64) for g, v in res[1].items()}, {g: int(v) for g, v in res[2].items()}),
                       restated, key)
        pack(out, key, df, paired, layout, res)
        out[key + '_census'] = np.array([restated[3][c] for c in ro.CENSUS_KEYS], dtype=np.int64)
        total.append(restated[3])
        print(key, what, 'paired' if paired else 'single', len(df), 'rows; counted', int(out[key + '_counts'].sum()))
    total = ro.merge_census(total)
    print('census of the edge cases:', dict(total))
    missing = [c for c in ro.CENSUS_KEYS if total[c] == 0 and c not in ('negative_bound', 'iso_gap_drop')]
    assert not missing and total['nseg_max'] >= 4, missing
    path = os.path.join(ROOT, 'tests', 'golden', 'reads_edges.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


def main(ref_root):
    sys.modules.setdefault('pysam', types.ModuleType('pysam'))
    sys.path.insert(0, ref_root)
    from degnorm import reads as R
    out = {}
    cases = [('se', rf.synth_reads(1, rf.golden_layout(), 3000), False, rf.golden_layout()),
             ('pe', rf.synth_pairs(2, rf.golden_layout(), 2000), True, rf.golden_layout()),
             ('qi', rf.synth_reads(3, rf.quiet_layout(), 400, skip=('R',), noise=0.0), False, rf.quiet_layout())]
    for key, df, paired, layout in cases:
        with tempfile.TemporaryDirectory() as d:
            res = run_reference(R, df, paired, layout, d)
        pack(out, key, df, paired, layout, res)
        print(key, len(df), 'rows; counts', out[key + '_counts'].tolist(), 'nnz', out[key + '_csr_idx'].size)
    cig, starts = rf.fuzz_cigars(4, 4000)
    bounds, nseg = [], []
    for c, s in zip(cig, starts.tolist()):
        try:
            b = R.cigar_segment_bounds(c, s)
        except ValueError:
            b = []
        nseg.append(len(b) // 2)
        bounds += b
    enc = [c.encode() for c in cig]
    out['fz_cig'] = np.frombuffer(b''.join(enc), dtype=np.uint8)
    out['fz_cig_off'] = np.r_[0, np.cumsum([len(e) for e in enc])].astype(np.int64)
    out['fz_pos'] = starts.astype(np.int64)
    out['fz_nseg'] = np.array(nseg, dtype=np.int32)
    out['fz_bounds'] = np.array(bounds, dtype=np.int64)
    out['fz_end_pos'] = np.array([s + sum(int(k) for k, _ in R.re.findall(r'(\d+)([A-Z]?)', c)) for c, s in zip(cig, starts.tolist())],
                                 dtype=np.int64)
    path = os.path.join(ROOT, 'tests', 'golden', 'reads.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    edge_cases(R)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('DEGNORM_REF', '../DegNorm'))
