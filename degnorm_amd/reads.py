"""
Per-sample chromosome coverage and gene read counts on the device (reference: `degnorm/reads.py`).

The reference's `BamReadsProcessor.chromosome_coverage_read_counts` (reads.py:314-818) walks every read of a chromosome
in Python: CIGAR parse, exon-union filter, full-inclusion test against the genes of the read's overlap group, isolated
gene lookup and a fancy-index `+= 1` per read.  Here the host packs the reads and the annotation into flat arrays and
one call, `dn_read_coverage` (csrc/dn_reads.hip), does all of it on the GPU; only the CSR nonzeros, the overlap genes'
span vectors and the counts come back.

    chromosome_coverage_read_counts_df(reads_df, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df, paired)
                                         -> (CSR row or None, {overlap gene: coverage}, {gene: read count})
    BamReadsProcessor                    the reference's class: same constructor, methods and output files

The host helpers `cigar_segment_bounds`, `fill_in_bounds` and `BamReadsProcessor.determine_full_inclusion` keep the
reference's signatures and semantics.  Opening BAM files needs pysam; without it the BAM-facing methods raise ImportError.
"""
import ctypes
import logging
import os
import pickle as pkl
import re

import numpy as np

from . import _lib
from ._lib import _p as _ptr

_TOKEN = re.compile(r'(\d+)([A-Z]?)')


def cigar_segment_bounds(cigar, start):
    """
    Inclusive [start, end] bounds of a read's match (M) runs, flattened: '50M25N50M' at 100 -> [100, 149, 175, 224].

    Every op other than M (a digit run not followed by a capital letter, e.g. '=', included) only advances the position,
    by one more when it directly follows an M; an M run of length L advances it by L - 1.  Raises ValueError when the
    CIGAR string has no M op.
    """
    out = []
    after_match = False
    for num, op in _TOKEN.findall(cigar):
        length = int(num)
        if op == 'M':
            out += [start, start + length - 1]
            start += length - 1
            after_match = True
        else:
            start += length + 1 if after_match else length
            after_match = False
    if not out:
        raise ValueError('CIGAR string {0} has no matching region.'.format(cigar))
    return out


def cigar_length(cigar):
    """Sum of all op lengths of a CIGAR string: end_pos = pos + cigar_length(cigar) (reference reads.py:404-405)."""
    return sum(int(num) for num, _ in _TOKEN.findall(cigar))


def fill_in_bounds(bounds_vec, endpoint=False):
    """
    Integers of the regions outlined by consecutive (start, end) pairs: [10, 13, 20, 24] -> [10, 11, 12, 20, ..., 23];
    with endpoint=True each end is included.  Raises ValueError for an odd number of bounds.
    """
    n = len(bounds_vec)
    if n % 2 != 0:
        raise ValueError('bounds_vec = {0}, must have even number of values!'.format(bounds_vec))
    extra = 1 if endpoint else 0
    return np.concatenate([np.arange(bounds_vec[j], bounds_vec[j + 1] + extra) for j in range(0, n, 2)])


def _merge_half_open(lo, hi):
    """Union of half-open [lo, hi) intervals (touching ones merged) as closed (lo, hi) rows, sorted."""
    keep = hi > lo
    lo, hi = lo[keep], hi[keep]
    if lo.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    o = np.argsort(lo, kind='stable')
    lo, hi = lo[o], hi[o]
    run_end = np.maximum.accumulate(hi)
    new = np.ones(lo.size, dtype=bool)
    new[1:] = lo[1:] > run_end[:-1]
    starts = np.flatnonzero(new)
    ends = np.append(starts[1:], lo.size) - 1
    return np.stack([lo[starts], run_end[ends] - 1], axis=1).astype(np.int64)


def pack_reads(reads_df, paired):
    """Host side of the device call: positions, CIGAR bytes + offsets and (paired) pair ids of the rows, in row order."""
    cig = reads_df['cigar'].tolist()
    pos = np.ascontiguousarray(reads_df['pos'].values, dtype=np.int64)
    enc = [c.encode('ascii') for c in cig]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
    buf = np.frombuffer(b''.join(enc), dtype=np.uint8) if off[-1] > 0 else np.zeros(1, dtype=np.uint8)
    pair_id, n_ids = None, 0
    if paired:
        import pandas as pd
        codes, uniq = pd.factorize(reads_df['qname_unpaired'])
        pair_id, n_ids = np.ascontiguousarray(codes, dtype=np.int32), len(uniq)
    return pos, off, np.ascontiguousarray(buf), pair_id, n_ids


class Annotation(object):
    """One chromosome's genes and exons in the flat layout dn_read_coverage takes (include/degnorm_amd.h)."""

    def __init__(self, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df):
        self.genes = chrom_gene_df['gene'].tolist()
        gidx = {g: k for k, g in enumerate(self.genes)}
        iso = list(gene_overlap_dat['isolated_genes'] or [])
        groups = [list(g) for g in (gene_overlap_dat['overlap_genes'] or [])]
        if len(iso) + sum(len(g) for g in groups) != len(self.genes):
            raise ValueError('number of genes contained in gene_overlap_dat does not match that of chrom_gene_df.')
        chrom_len = int(chrom_len)
        if not 0 < chrom_len < 2 ** 31 - 4:
            raise ValueError('chromosome length {0} outside 1 .. 2^31 - 5'.format(chrom_len))
        gs = chrom_gene_df['gene_start'].values.astype(np.int64)
        ge = chrom_gene_df['gene_end'].values.astype(np.int64)
        es = chrom_exon_df['start'].values.astype(np.int64)
        ee = chrom_exon_df['end'].values.astype(np.int64)
        if (gs.size and (gs.min() < 1 or ge.max() > chrom_len)) or (es.size and (es.min() < 1 or ee.max() > chrom_len)):
            raise ValueError('gene or exon coordinates outside the chromosome (1 .. {0})'.format(chrom_len))
        self.chrom_len = chrom_len
        # position pre-filter (reads.py:412-413) and the exon union the reference marks in tscript_vec (:432-435)
        self.keep_lo = int(gs.min()) - 1 if gs.size else 0
        self.keep_hi = int(ge.max()) - 1 if ge.size else -1
        self.exon_iv = _merge_half_open(es - 1, ee)
        self.exon_union_len = int((self.exon_iv[:, 1] - self.exon_iv[:, 0] + 1).sum())
        # overlap groups: disjoint spans [min gene_start - 1, max gene_end - 1] (:551-552), sorted
        span = {g: (int(a) - 1, int(b) - 1) for g, a, b in zip(self.genes, gs, ge)}
        self.groups = groups
        g_iv = np.array([[min(span[g][0] for g in grp), max(span[g][1] for g in grp)] for grp in groups],
                        dtype=np.int64).reshape(-1, 2)
        g_order = np.argsort(g_iv[:, 0], kind='stable')
        self.group_iv = np.ascontiguousarray(g_iv[g_order])
        if len(groups) > 1 and (self.group_iv[1:, 0] <= self.group_iv[:-1, 1]).any():
            raise ValueError('overlap groups of gene_overlap_dat have intersecting spans')
        exon_rows = chrom_exon_df.groupby('gene', sort=False).indices if len(chrom_exon_df) else {}
        egs = chrom_exon_df['gene_start'].values.astype(np.int64) if len(chrom_exon_df) else np.zeros(0, np.int64)
        ege = chrom_exon_df['gene_end'].values.astype(np.int64) if len(chrom_exon_df) else np.zeros(0, np.int64)
        ol_gene, ol_gs0, cov_off, ex_off, ex_b, grp_off = [], [], [0], [0], [], [0]
        self.ol_names, self.ol_tidx = [], []
        for k in g_order.tolist():
            for g in groups[k]:
                rows = exon_rows.get(g)
                if rows is None or len(rows) == 0:
                    raise ValueError('overlap gene {0} has no exons in chrom_exon_df'.format(g))
                gs0, ge0 = int(egs[rows[0]]) - 1, int(ege[rows[0]]) - 1      # :565-566
                e0, e1 = np.sort(es[rows]) - 1, np.sort(ee[rows])            # separately sorted starts and ends (:575)
                if e0.min() < gs0 or e1.max() > ge0 + 1:
                    raise ValueError('exons of overlap gene {0} reach outside its gene span'.format(g))
                ol_gene.append(gidx[g])
                ol_gs0.append(gs0)
                cov_off.append(cov_off[-1] + (ge0 - gs0 + 1) + 1)                 # span vector + one pad slot
                ex_b.append(np.stack([e0, e1], axis=1))
                ex_off.append(ex_off[-1] + len(rows))
                self.ol_names.append(g)
                self.ol_tidx.append(np.unique(np.concatenate([np.arange(a, b) for a, b in zip(e0, e1)])) - gs0)  # :577, :644
            grp_off.append(len(ol_gene))
        self.group_gene_off = np.array(grp_off, dtype=np.int32)
        self.ol_gene = np.array(ol_gene, dtype=np.int32)
        self.ol_gs0 = np.array(ol_gs0, dtype=np.int64)
        self.ol_cov_off = np.array(cov_off, dtype=np.int64)
        self.ol_exon_off = np.array(ex_off, dtype=np.int32)
        self.ol_exon = np.ascontiguousarray(np.concatenate(ex_b).astype(np.int64)) if ex_b else np.zeros((0, 2), np.int64)
        # isolated genes: closed spans [gene_start - 1, gene_end - 1] (:685-688, :723-728) and their union
        iso_lo = np.array([span[g][0] for g in iso], dtype=np.int64)
        iso_hi = np.array([span[g][1] for g in iso], dtype=np.int64)
        o = np.argsort(iso_lo, kind='stable')
        self.iso_iv = np.ascontiguousarray(np.stack([iso_lo[o], iso_hi[o]], axis=1)) if iso else np.zeros((0, 2), np.int64)
        if len(iso) > 1 and (self.iso_iv[1:, 0] <= self.iso_iv[:-1, 1]).any():
            raise ValueError('isolated genes of gene_overlap_dat overlap each other')
        self.iso_gene = np.array([gidx[g] for g in iso], dtype=np.int32)[o] if iso else np.zeros(0, np.int32)
        self.iso_union = _merge_half_open(iso_lo, iso_hi + 1)
        self.n_isolated, self.n_overlap = len(iso), len(ol_gene)


def check_coverage_call(rc, what):
    """
    _lib._check for the coverage calls.  A kept row with more than DN_READS_MAX_SEG M ops (DN_E_UNSUPPORTED) is a fault of
    the caller's data, as a CIGAR without an M op is: ValueError with the library's text, which names the CIGAR.
    """
    if rc == _lib.DN_E_UNSUPPORTED:
        raise ValueError(_lib.load().dn_last_error().decode('utf-8', 'replace'))
    _lib._check(rc, what)


STRANDED = ('no', 'forward', 'reverse')
STRANDS = ('+', '-')


def check_stranded(stranded):
    """ValueError unless stranded is 'no', 'forward' or 'reverse' (the rule: include/degnorm_amd.h, "Strand-specific counting")."""
    if not isinstance(stranded, str) or stranded not in STRANDED:
        raise ValueError('stranded must be {0}, not {1!r}'.format(' or '.join(repr(m) for m in STRANDED), stranded))
    return stranded


def check_strand(strand):
    """ValueError unless strand is '+' or '-'; its byte."""
    if not isinstance(strand, str) or strand not in STRANDS:
        raise ValueError("strand must be '+' or '-', not {0!r}".format(strand))
    return ord(strand)


def row_sense(flag, names, by_name, stranded):
    """
    The sense ('+' / '-') of rows with these FLAGs and names under protocol `stranded` ('forward' or 'reverse'), by the
    library's host build of the record rule (dn_read_sense_host; no device needed).  by_name: the rows are those of a store
    paired by the name rule, where a name ending in '2' also marks a last mate.
    """
    if check_stranded(stranded) == 'no':
        raise ValueError("rows have a sense under 'forward' or 'reverse' only")
    flag = np.ascontiguousarray(flag, dtype=np.uint16).reshape(-1)
    n = len(flag)
    if len(names) != n:
        raise ValueError('row_sense: one name per FLAG')
    last = np.array([(x if isinstance(x, bytes) else str(x).encode('ascii', 'replace'))[-1:] or b'\0' for x in names] or [b'\0'],
                    dtype='S1').view(np.uint8)
    out = np.zeros(max(n, 1), dtype=np.uint8)
    f = flag if n else np.zeros(1, np.uint16)
    _lib._check(_lib.load().dn_read_sense_host(n, _ptr(f, ctypes.c_uint16), _ptr(last, ctypes.c_uint8), 1 if by_name else 0,
                                               STRANDED.index(stranded), _ptr(out, ctypes.c_uint8)), 'dn_read_sense_host')
    return [chr(c) for c in out[:n].tolist()]


def pack_sense(sense, n_rows):
    """The per-row sense column ('+' / '-' strings, or their bytes) as the uint8 array dn_read_coverage_strand takes."""
    a = np.asarray(sense)
    if a.dtype.kind in 'US' or a.dtype == object:
        a = np.array([ord(s) if isinstance(s, str) and len(s) == 1 else s[0] if isinstance(s, bytes) and len(s) == 1 else 0
                      for s in a.tolist()], dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    if len(a) != n_rows or not np.isin(a, (ord('+'), ord('-'))).all():
        raise ValueError("sense must hold '+' or '-' for every row")
    return a if n_rows else np.zeros(1, np.uint8)


def device_read_coverage(pos, off, cig, pair_id, n_ids, ann, paired, device=None, sense=None, strand=None):
    """
    One dn_read_coverage call on packed reads and an Annotation: (counts int64[n_genes], overlap span vectors int64 with
    their pad slots, CSR indices int32, CSR values int64, number of reads that reached the isolated stage, device ms).
    With `sense` (uint8 per row) and `strand` ('+' / '-') it is dn_read_coverage_strand: the position pre-filter keeps
    only the rows of that sense.
    """
    if (sense is None) != (strand is None):
        raise ValueError('sense and strand go together')
    lib = _lib.load()
    i32, i64, u8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint8
    n_genes = len(ann.genes)
    counts = np.zeros(max(n_genes, 1), dtype=np.int64)
    ol_cov = np.zeros(max(int(ann.ol_cov_off[-1]), 1), dtype=np.int64)
    cap = max(ann.exon_union_len, 1)
    csr_idx = np.zeros(cap, dtype=np.int32)
    csr_val = np.zeros(cap, dtype=np.int64)
    nnz, n_iso_reads, ms = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0.0)
    dev = int(os.environ.get('LOCAL_RANK', 0)) if device is None else int(device)
    n_groups = len(ann.group_iv)
    rows = (dev, 1 if paired else 0, len(pos), _ptr(pos, i64), _ptr(off, i64), _ptr(cig, u8), _ptr(pair_id, i32), int(n_ids))
    rest = (ann.chrom_len, ann.keep_lo, ann.keep_hi,
            len(ann.exon_iv), _ptr(ann.exon_iv, i64),
            n_groups, _ptr(ann.group_iv, i64), _ptr(ann.group_gene_off, i32),
            _ptr(ann.ol_gene, i32), _ptr(ann.ol_gs0, i64), _ptr(ann.ol_cov_off, i64),
            _ptr(ann.ol_exon_off, i32), _ptr(ann.ol_exon, i64),
            len(ann.iso_iv), _ptr(ann.iso_iv, i64), _ptr(ann.iso_gene, i32),
            len(ann.iso_union), _ptr(ann.iso_union, i64),
            n_genes, _ptr(counts, i64), _ptr(ol_cov, i64), cap, ctypes.byref(nnz),
            _ptr(csr_idx, i32), _ptr(csr_val, i64), ctypes.byref(n_iso_reads), ctypes.byref(ms))
    if strand is None:
        check_coverage_call(lib.dn_read_coverage(*(rows + rest)), 'dn_read_coverage')
    else:
        sense = pack_sense(sense, len(pos))
        sel = (_ptr(sense, u8), check_strand(strand))
        check_coverage_call(lib.dn_read_coverage_strand(*(rows + sel + rest)), 'dn_read_coverage_strand')
    k = int(nnz.value)
    return counts[:n_genes], ol_cov, csr_idx[:k].copy(), csr_val[:k].copy(), int(n_iso_reads.value), float(ms.value)


def device_cigar_bounds(cigars, starts, max_seg=16, device=None):
    """Device CIGAR parser (dn_reads_cigar_bounds): per string the flat bounds list (None: no M op) and end_pos."""
    import pandas as pd
    pos, off, cig, _, _ = pack_reads(pd.DataFrame({'pos': np.asarray(starts, dtype=np.int64), 'cigar': list(cigars)}), False)
    n = len(pos)
    nseg = np.zeros(max(n, 1), dtype=np.int32)
    bounds = np.zeros(max(n, 1) * 2 * max_seg, dtype=np.int64)
    end_pos = np.zeros(max(n, 1), dtype=np.int64)
    lib = _lib.load()
    rc = lib.dn_reads_cigar_bounds(int(os.environ.get('LOCAL_RANK', 0)) if device is None else int(device), n,
                                   _ptr(pos, ctypes.c_int64), _ptr(off, ctypes.c_int64), _ptr(cig, ctypes.c_uint8), int(max_seg),
                                   _ptr(nseg, ctypes.c_int32), _ptr(bounds, ctypes.c_int64), _ptr(end_pos, ctypes.c_int64))
    _lib._check(rc, 'dn_reads_cigar_bounds', invalid_is_value_error=False)
    b = bounds.reshape(max(n, 1), 2 * max_seg)
    out = [b[r, :2 * nseg[r]].tolist() if nseg[r] > 0 else None for r in range(n)]
    if (nseg[:n] < 0).any():
        raise ValueError('a CIGAR string has more than {0} match segments'.format(max_seg))
    return out, end_pos[:n]


def chromosome_coverage_read_counts_df(reads_df, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df, paired,
                                       device=None, sense=None, strand=None):
    """
    Coverage and read counts of one sample's reads on one chromosome, on the GPU: the computation of the reference's
    chromosome_coverage_read_counts (reads.py:389-805) without the file I/O.

    :param reads_df: the reads in the order they are taken: `pos` (0-based), `cigar`, and `qname_unpaired` when paired
    (pairs are consecutive rows, after the position pre-filter and the rule that a pair id occurs exactly twice).
    :param sense, strand: strand-specific counting (both or neither): `sense` holds '+' or '-' for every row of reads_df
    and `strand` is the one counted -- the position pre-filter also drops the rows of the other sense.  The annotation
    given is that strand's own.
    :return: (scipy.sparse.csr_matrix 1 x chrom_len of int64 -- the isolated genes' chromosome coverage -- or None when no
    read reached the isolated stage; {overlap gene: int64 coverage over its exon positions} in gene_overlap_dat order;
    {gene: read count} in chrom_gene_df order)
    """
    ann = Annotation(chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df)
    pos, off, cig, pair_id, n_ids = pack_reads(reads_df, paired)
    counts, ol_cov, idx, val, n_iso_reads, _ = device_read_coverage(pos, off, cig, pair_id, n_ids, ann, paired, device, sense, strand)
    return coverage_outputs(ann, counts, ol_cov, idx, val, n_iso_reads)


def coverage_outputs(ann, counts, ol_cov, idx, val, n_iso_reads):
    """The results of one device coverage call in the reference's form: (CSR row or None, {overlap gene: coverage}, counts)."""
    from scipy import sparse
    ol_span = {}
    for q, g in enumerate(ann.ol_names):
        ol_span[g] = ol_cov[ann.ol_cov_off[q]:ann.ol_cov_off[q + 1] - 1][ann.ol_tidx[q]]
    ol_cov_dict = {g: ol_span[g] for grp in ann.groups for g in grp}
    read_counts = {g: int(c) for g, c in zip(ann.genes, counts.tolist())}
    csr = None
    if ann.n_isolated > 0 and n_iso_reads > 0:
        csr = sparse.csr_matrix((val, idx, np.array([0, idx.size], dtype=np.int32)), shape=(1, ann.chrom_len))
    return csr, ol_cov_dict, read_counts


def _require_pysam():
    try:
        import pysam
    except ImportError as e:
        raise ImportError('reading .bam files needs pysam, which is not installed ({0}); load the reads yourself and '
                          'call degnorm_amd.reads.chromosome_coverage_read_counts_df'.format(e))
    return pysam


def reads_frame(rows, paired):
    """The reference's reads DataFrame from (qname, pos, cigar) rows in file order: `qname_unpaired` added and the rows
    sorted by it (pandas' default quicksort) when paired."""
    from pandas import DataFrame
    df = DataFrame(rows, columns=['qname', 'pos', 'cigar'])
    df['pos'] = df['pos'].astype('int')
    if paired:
        df['qname_unpaired'] = df.qname.apply(lambda x: '.'.join(x.split('.')[:-1]))
        df.sort_values('qname_unpaired', inplace=True)
    return df


class BamReadsProcessor(object):
    index_extensions = ('.bai',)                 # what the backend that opens the file can read

    def __init__(self, bam_file, index_file, chroms=None, n_jobs=1, output_dir=None, unique_alignment=True, verbose=True,
                 stranded='no'):
        """
        Coverage and read counts of one alignment file (.bam), as the reference's BamReadsProcessor (reads.py:97-136).
        Needs pysam to open the file (ImportError without it).  n_jobs is kept for the signature: chromosomes run one
        after another, each as one device call.  This reader does not count by strand: any `stranded` but 'no' is a
        ValueError (bam.NativeBamReadsProcessor has the option).
        """
        if check_stranded(stranded) != 'no':
            raise ValueError('strand-specific counting (stranded={0!r}) needs bam.NativeBamReadsProcessor'.format(stranded))
        self.filename = bam_file
        if not output_dir:
            output_dir = os.path.join(os.path.dirname(self.filename), 'tmp')
        self.index_filename = index_file
        self.n_jobs = n_jobs
        self.verbose = verbose
        self.sample_id = '.'.join(os.path.basename(self.filename).split('.')[:-1])
        self.save_dir = os.path.join(output_dir, self.sample_id)
        self.header = None
        self.paired = None
        self.chroms = chroms
        self.unique_alignment = unique_alignment
        self._open_backend()
        if not os.path.isfile(bam_file) or not bam_file.endswith('.bam'):
            raise ValueError('{0} is not a .bam file'.format(bam_file))
        if not os.path.isfile(index_file):
            raise FileNotFoundError('{0} .bam index file not found'.format(index_file))
        if not index_file.endswith(self.index_extensions):
            raise ValueError('.bam index file does not have correct .bai file extension.')
        self.get_header()
        self.determine_if_paired()
        if self.verbose:
            logging.info('SAMPLE {0} -- sample contains {1} reads'.format(self.sample_id, 'paired' if self.paired else 'single-end'))

    def _open_backend(self):
        """What reading the file needs, checked before the file itself: pysam."""
        self._pysam = _require_pysam()

    def _open(self):
        pysam = getattr(self, '_pysam', None) or _require_pysam()
        return pysam.AlignmentFile(self.filename, 'rb', index_filename=self.index_filename)

    def get_header(self):
        """self.header: DataFrame of `chr`, `length` from the .bam header; self.chroms: requested chromosomes in it."""
        from pandas import DataFrame
        lengths = self._reference_lengths()
        self.header = DataFrame(list(lengths.items()), columns=['chr', 'length'])
        if self.chroms is not None:
            self.chroms = np.intersect1d(self.chroms, self.header.chr.unique()).tolist()
        else:
            self.chroms = self.header.chr.unique().tolist()

    def _reference_lengths(self):
        """{SQ name: length} of the .bam header."""
        bam = self._open()
        sq = bam.header.to_dict().get('SQ', [])
        bam.close()
        return {h.get('SN'): h.get('LN') for h in sq}

    def _leading_query_names(self, chrom):
        """Query names of the first 301 reads of chrom, in file order, unfiltered."""
        bam = self._open()
        names = []
        for read in bam.fetch(chrom):
            names.append(read.query_name)
            if len(names) > 300:
                break
        bam.close()
        return names

    def determine_if_paired(self):
        """Paired when the query names of the first ~300 reads end in exactly the suffixes .1 and .2."""
        self.paired = False
        names = self._leading_query_names(self.chroms[0])
        self.paired = set(x.split('.')[-1] for x in names) == {'1', '2'}

    def load_chromosome_reads(self, chrom):
        """
        DataFrame of `qname`, `pos`, `cigar` (and `qname_unpaired`, sorted by it, when paired) of one chromosome's reads;
        reads with NH > 1 are skipped when unique_alignment, unpaired reads (RNEXT '*') when paired.
        """
        rows = []
        bam = self._open()
        for read in bam.fetch(chrom):
            if self.unique_alignment and read.has_tag('NH') and read.get_tag('NH') > 1:
                continue
            if self.paired and read.next_reference_id == -1:
                continue
            rows.append((read.query_name, read.reference_start, read.cigarstring))
        bam.close()
        return reads_frame(rows, self.paired)

    @staticmethod
    def determine_full_inclusion(read_bounds, gene_exon_bounds):
        """
        Indices of the genes whose exons fully capture every match region of a read: region [s, e] is captured by a gene
        when one of its [exon start, exon end] bounds has start <= s and e <= end.

        :param read_bounds: flat list of region starts and ends (inclusive).
        :param gene_exon_bounds: per gene, a list of [exon start, exon end] pairs.
        """
        regions = [(read_bounds[j], read_bounds[j + 1]) for j in range(0, len(read_bounds) - 1, 2)]
        return [k for k, exons in enumerate(gene_exon_bounds)
                if all(any(s >= lo and e <= hi for lo, hi in exons) for s, e in regions)]

    def _files(self, chrom):
        tag = self.sample_id + '_' + str(chrom)
        return (os.path.join(self.save_dir, 'chrom_coverage_' + tag + '.npz'),
                os.path.join(self.save_dir, 'overlap_coverage_' + tag + '.pkl'),
                os.path.join(self.save_dir, 'read_counts_' + tag + '.csv'))

    def chromosome_coverage_read_counts(self, gene_overlap_dat, chrom_gene_df, chrom_exon_df, chrom):
        """
        Coverage and read counts of one chromosome (reference reads.py:314-818), written to self.save_dir:
        chrom_coverage_<sample>_<chr>.npz (the isolated genes' coverage as a 1 x chrom_len CSR row; not written when no
        read reaches the isolated stage), overlap_coverage_<sample>_<chr>.pkl ({overlap gene: exon coverage}) and
        read_counts_<sample>_<chr>.csv (columns gene, <sample>).  When every file this chromosome needs already exists,
        nothing is computed (reads.py:374-386).
        """
        from pandas import DataFrame
        from scipy import sparse
        verbose = getattr(self, 'verbose', False)
        n_iso = len(gene_overlap_dat['isolated_genes'] or [])
        n_ol = int(sum(len(g) for g in (gene_overlap_dat['overlap_genes'] or [])))
        if n_iso + n_ol != chrom_gene_df.shape[0]:
            raise ValueError('number of genes contained in gene_overlap_dat does not match that of chrom_gene_df.')
        chrom_cov_file, ol_cov_file, count_file = self._files(chrom)
        if (n_iso == 0 or os.path.isfile(chrom_cov_file)) and (n_ol == 0 or os.path.isfile(ol_cov_file)) \
                and os.path.isfile(count_file):
            if verbose:
                logging.info('SAMPLE {0}, CHR {1} -- all coverage and read count files already present; skipping.'
                             .format(self.sample_id, chrom))
            return None
        chrom_len = int(self.header[self.header.chr == chrom].length.iloc[0])
        csr, ol_cov_dict, read_counts, n_reads = self._chromosome_coverage(chrom, chrom_len, gene_overlap_dat, chrom_gene_df,
                                                                           chrom_exon_df)
        if n_ol > 0:
            with open(ol_cov_file, 'wb') as f:
                pkl.dump(ol_cov_dict, f)
        if csr is not None:
            sparse.save_npz(chrom_cov_file, matrix=csr)
        DataFrame({'gene': list(read_counts.keys()), self.sample_id: list(read_counts.values())}).to_csv(count_file, index=False)
        if verbose:
            logging.info('SAMPLE {0}, CHR {1} -- {2} reads, {3} counted{4}'.format(
                self.sample_id, chrom, n_reads, sum(read_counts.values()), getattr(self, '_chrom_note', '')))
        return None

    def _chromosome_coverage(self, chrom, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df):
        """(CSR row or None, overlap coverage, read counts, number of reads loaded) of one chromosome."""
        reads_df = self.load_chromosome_reads(chrom)
        csr, ol_cov_dict, read_counts = chromosome_coverage_read_counts_df(
            reads_df, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df, self.paired)
        return csr, ol_cov_dict, read_counts, reads_df.shape[0]

    def coverage_read_counts(self, gene_overlap_dict, gene_df, exon_df):
        """chromosome_coverage_read_counts for every chromosome of self.chroms (reference reads.py:820-847)."""
        if not os.path.exists(self.save_dir):
            os.makedirs(self.save_dir)
        for chrom in self.chroms:
            self.chromosome_coverage_read_counts(gene_overlap_dat=gene_overlap_dict.get(chrom),
                                                 chrom_gene_df=gene_df[gene_df.chr.isin([chrom])],
                                                 chrom_exon_df=exon_df[exon_df.chr.isin([chrom])],
                                                 chrom=chrom)
