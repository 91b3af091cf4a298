"""
A full restatement of the reads -> coverage / read counts rules (test tooling, CPU only; not product code).

`restate` computes what the reference's chromosome_coverage_read_counts (reads.py:397-786) computes, for any CIGAR, single-end
and paired, with plain Python loops over whole-chromosome numpy vectors: no intervals, no binary searches and nothing of
degnorm_amd.reads but its CIGAR parser (`cigar_segment_bounds` / `cigar_length`, held to the reference's fuzz golden by
tests/test_reads_host.py).  It is written from the rules, so it checks the host packing (`reads.Annotation`) together with
the kernels.  tests/test_reads_oracle_host.py holds it to the reference's own outputs (tests/golden/reads.npz,
tests/golden/reads_edges.npz).

One rule is the library's and not the reference's: a unit (a read, or a pair) with a segment bound below 0 is dropped
(`negative_bound`); the reference indexes from the end of its vectors there.

Every unit also leaves a mark in `census` for each branch it took, so that a test can assert that its cases still reach
the branches they were built for:

  prefilter_drop            rows outside [first gene start, last gene end]
  pair_id_once / _thrice    pair ids that occur once / three or more times among the rows left (their rows are dropped)
  pair_not_adjacent         pairs (consecutive survivors) whose two rows carry different pair ids
  clip_right_changed        mate 2 reaches at least as far right as mate 1 and the clip changed a bound
  clip_left_changed         mate 2 ends left of mate 1's end and the clip changed a bound
  clip_left_resorted        ... and sorting the clipped bounds changed their order (needs a zero-length M op)
  empty_segment             units with a segment whose end is below its start
  negative_bound            units dropped for a bound below 0
  exon_drop                 units with a segment that leaves the exon union
  caught_0 / _1 / _2plus    units inside an overlap group's span by the number of its genes that capture every segment
  group_fallthrough_to_iso  units no gene of their group captured: they go on to the isolated stage (== caught_0)
  wrap                      counted overlap units with a position on the gene's first base (index -1: the last slot)
  wrap_only_piece           ... of which a whole segment is that one base (nothing of it is left but the wrapped slot)
  ol_runs_merged            counted overlap units of which two pieces overlap or touch (fewer runs than pieces)
  iso_union_drop            units whose [pos, end_pos] leaves the union of the isolated genes' spans
  iso_gap_drop              units inside that union whose pos lies in no isolated gene.  Always 0: the union is made of
                            exactly the genes' positions, so the branch (the reference's KeyError path, :735-761) is dead
  iso_on_gene_last_base     counted isolated units whose pos is the last base of their gene (the edge of that branch)
  iso_spans_touching_genes  counted isolated units whose end_pos lies past their gene's end (touching genes)
  iso_runs_merged           counted isolated units of which two segments overlap or touch
  nseg_max                  not a count: the largest number of M ops of a row left after the pre-filter (and pair rule)
"""
import collections

import numpy as np

from degnorm_amd.reads import cigar_length, cigar_segment_bounds

CENSUS_KEYS = ('prefilter_drop', 'pair_id_once', 'pair_id_thrice', 'pair_not_adjacent',
               'clip_right_changed', 'clip_left_changed', 'clip_left_resorted', 'empty_segment',
               'negative_bound', 'exon_drop',
               'caught_0', 'caught_1', 'caught_2plus', 'group_fallthrough_to_iso', 'wrap', 'wrap_only_piece', 'ol_runs_merged',
               'iso_union_drop', 'iso_gap_drop', 'iso_on_gene_last_base', 'iso_spans_touching_genes', 'iso_runs_merged',
               'nseg_max')


def merge_census(censuses):
    """Sum of censuses; `nseg_max` is their maximum."""
    total = collections.Counter({k: 0 for k in CENSUS_KEYS})
    for c in censuses:
        for k, v in c.items():
            total[k] = max(total[k], v) if k == 'nseg_max' else total[k] + v
    return total


def _runs(idx):
    """Number of maximal runs of consecutive integers in a sorted array of distinct integers."""
    return int(idx.size > 0) + int((np.diff(idx) > 1).sum())


def _pair_bounds(b1, b2, census):
    """Mate 2's bounds clipped against mate 1's extent (:460-467), appended to mate 1's."""
    lo1, hi1, hi2 = min(b1), max(b1), max(b2)
    if hi2 >= hi1:
        clipped = [hi1 + 1 if v <= hi1 else v for v in b2]
        census['clip_right_changed'] += clipped != b2
    else:
        clipped = [lo1 - 1 if v >= lo1 else v for v in b2]
        census['clip_left_changed'] += clipped != b2
        census['clip_left_resorted'] += sorted(clipped) != clipped
        clipped.sort()
    return b1 + clipped


def restate(reads_df, chrom_len, gene_overlap_dat, gene_df, exon_df, paired, trace=None):
    """
    (CSR row or None, {overlap gene: coverage}, {gene: count}, census) of one chromosome's reads.  With a dict as `trace`,
    trace['negative_rows'] becomes the row numbers (positions in reads_df) of the units dropped for a bound below 0.
    """
    from scipy import sparse
    census = collections.Counter({k: 0 for k in CENSUS_KEYS})
    chrom_len = int(chrom_len)
    pos = [int(v) for v in reads_df['pos'].values]
    cigar = [str(c) for c in reads_df['cigar'].values]
    end = [p + cigar_length(c) for p, c in zip(pos, cigar)]
    genes = gene_df['gene'].tolist()
    start_of = {g: int(v) for g, v in zip(genes, gene_df['gene_start'].values)}
    end_of = {g: int(v) for g, v in zip(genes, gene_df['gene_end'].values)}
    counts = {g: 0 for g in genes}

    # rows between the first gene's start and the last gene's end (0-based); then ids that occur exactly twice
    first, last = min(start_of.values()) - 1, max(end_of.values()) - 1
    rows = [r for r in range(len(pos)) if pos[r] >= first and end[r] <= last]
    census['prefilter_drop'] = len(pos) - len(rows)
    if paired:
        ids = reads_df['qname_unpaired'].tolist()
        seen = collections.Counter(ids[r] for r in rows)
        census['pair_id_once'] = sum(1 for n in seen.values() if n == 1)
        census['pair_id_thrice'] = sum(1 for n in seen.values() if n >= 3)
        rows = [r for r in rows if seen[ids[r]] == 2]
        units = [(rows[k], rows[k + 1]) for k in range(0, len(rows) - 1, 2)]
        census['pair_not_adjacent'] = sum(1 for a, b in units if ids[a] != ids[b])
    else:
        units = [(r,) for r in rows]

    # segments per unit; a unit keeps the pos / end_pos of its last row
    off_exon = np.ones(chrom_len, dtype=bool)
    for a, b in zip(exon_df['start'].values, exon_df['end'].values):
        off_exon[int(a) - 1:int(b)] = False
    alive, negative_rows = [], []
    for unit in units:
        per_row = [cigar_segment_bounds(cigar[r], pos[r]) for r in unit]
        census['nseg_max'] = max([census['nseg_max']] + [len(b) // 2 for b in per_row])
        flat = _pair_bounds(per_row[0], per_row[1], census) if paired else per_row[0]
        segs = list(zip(flat[0::2], flat[1::2]))
        census['empty_segment'] += any(b < a for a, b in segs)
        if min(flat) < 0:
            census['negative_bound'] += 1
            negative_rows += list(unit)
            continue
        if any(off_exon[a:b + 1].any() for a, b in segs):
            census['exon_drop'] += 1
            continue
        alive.append((pos[unit[-1]], end[unit[-1]], segs))
    if trace is not None:
        trace['negative_rows'] = negative_rows

    # overlap groups: a unit inside a group's span is counted for the one gene whose exons capture all its segments
    ol_cov = {}
    for group in gene_overlap_dat['overlap_genes'] or []:
        g_lo, g_hi = min(start_of[g] for g in group) - 1, max(end_of[g] for g in group) - 1
        exons, gene_lo, vec = {}, {}, {}
        for g in group:
            d = exon_df[exon_df['gene'] == g]
            gene_lo[g] = int(d['gene_start'].iloc[0]) - 1
            vec[g] = np.zeros(int(d['gene_end'].iloc[0]) - 1 - gene_lo[g] + 1, dtype=np.int64)
            # starts and ends are sorted apart and paired up again; an exon is [start - 1, end] here, end included
            exons[g] = list(zip((np.sort(d['start'].values) - 1).tolist(), np.sort(d['end'].values).tolist()))
        rest = []
        for p, e, segs in alive:
            if not (p >= g_lo and e <= g_hi):
                rest.append((p, e, segs))
                continue
            caught = [g for g in group if all(any(a >= x and b <= y for x, y in exons[g]) for a, b in segs)]
            census['caught_0' if not caught else 'caught_1' if len(caught) == 1 else 'caught_2plus'] += 1
            if not caught:
                census['group_fallthrough_to_iso'] += 1
                rest.append((p, e, segs))
            if len(caught) != 1:
                continue
            g = caught[0]
            counts[g] += 1
            # position x is counted in slot x - gene start - 1; slot -1 is the vector's last; once per unit and slot
            pieces = [np.arange(a, b + 1) - gene_lo[g] - 1 for a, b in segs if b >= a]
            idx = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int64)
            wrapped = bool((idx < 0).any())
            census['wrap'] += wrapped
            census['wrap_only_piece'] += any(x.max() < 0 for x in pieces)
            slots = np.unique(np.where(idx < 0, idx + vec[g].size, idx))
            n_pieces = sum(1 for x in pieces if x.max() >= 0) + wrapped
            census['ol_runs_merged'] += _runs(slots) < n_pieces
            vec[g][slots] += 1
        alive = rest
        for g in group:
            at = np.unique(np.concatenate([np.arange(x, y) for x, y in exons[g]])) - gene_lo[g]
            ol_cov[g] = vec[g][at]

    # isolated genes: [pos, end_pos] inside the union of their spans; the gene is the one holding pos
    iso = list(gene_overlap_dat['isolated_genes'] or [])
    csr = None
    if iso:
        owner = np.full(chrom_len, -1, dtype=np.int64)
        for k, g in enumerate(iso):
            owner[start_of[g] - 1:end_of[g]] = k
        cov = np.zeros(chrom_len, dtype=np.int64)
        n_counted = 0
        for p, e, segs in alive:
            if (owner[p:e + 1] < 0).any():
                census['iso_union_drop'] += 1
                continue
            if owner[p] < 0:
                census['iso_gap_drop'] += 1
                continue
            g = iso[owner[p]]
            counts[g] += 1
            n_counted += 1
            census['iso_on_gene_last_base'] += p == end_of[g] - 1
            census['iso_spans_touching_genes'] += e > end_of[g] - 1
            pieces = [np.arange(a, b + 1) for a, b in segs if b >= a]
            at = np.unique(np.concatenate(pieces)) if pieces else np.zeros(0, dtype=np.int64)
            census['iso_runs_merged'] += _runs(at) < len(pieces)
            cov[at] += 1
        if n_counted:
            csr = sparse.csr_matrix(cov)
    return csr, ol_cov, counts, census


def assert_same(got, want, what=''):
    """(csr, overlap coverage, counts) `got` equals `want` exactly: values, order of the dicts and the outputs' dtypes."""
    (csr, ol, counts), (csr_e, ol_e, counts_e) = got[:3], want[:3]
    assert (csr is None) == (csr_e is None), what
    if csr_e is not None:
        assert csr.dtype == np.int64 and csr.indices.dtype == np.int32 and csr.shape == csr_e.shape, what
        np.testing.assert_array_equal(csr.indices, csr_e.indices, err_msg=what)
        np.testing.assert_array_equal(csr.data, csr_e.data, err_msg=what)
    assert list(ol) == list(ol_e), what
    for g in ol_e:
        assert ol[g].dtype == np.int64, what
        np.testing.assert_array_equal(ol[g], ol_e[g], err_msg='{0} {1}'.format(what, g))
    assert list(counts) == list(counts_e) and counts == counts_e, what
