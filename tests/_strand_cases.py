"""
Strand-specific counting: plain-Python restatements and case builders (test tooling, CPU only; not product code).

The rule is in include/degnorm_amd.h, "Strand-specific counting".  Its guarantee makes the unstranded path the oracle: a
stranded run over annotation A and reads B gives, gene for gene, what the unstranded code gives on (A+, B+) and on
(A-, B-).  Here are

  sense_rule        the sense of one record, restated from the header's words
  split_tables      A+ and A-: each strand's genes, their exons and their own overlap structure
  split_reads       B+ and B-: the rows of each sense, in the order given
  expected          the restatement of tests/_reads_oracle.py on (A^s, B^s) for one strand
  hand_case         a hand-made annotation and reads with the counts written out: unstranded, forward, reverse
  stranded_case     a seeded annotation with a strand per gene and seeded reads with a sense per row
"""
import numpy as np
import pandas as pd

import _reads_fixtures as rf
import _reads_oracle as ro
from degnorm_amd.gene_processing import get_gene_overlap_structure

STRANDS = ('+', '-')
PROTOCOLS = ('forward', 'reverse')
STORE_KINDS = ('single', 'name', 'flag')            # single-end store, paired by the name rule, paired by FLAG


def sense_rule(flag, name, store, protocol):
    """'+' or '-' for a record with this FLAG and name in a store of kind `store` under `protocol`."""
    assert store in STORE_KINDS and protocol in PROTOCOLS
    last_mate = bool(flag & 0x1) and bool(flag & 0x80)
    if store == 'name' and name.endswith('2'):
        last_mate = True
    sense = '-' if flag & 0x10 else '+'
    flip = {'+': '-', '-': '+'}
    if last_mate:
        sense = flip[sense]
    if protocol == 'reverse':
        sense = flip[sense]
    return sense


def split_tables(gene_df, exon_df, strand_of):
    """{strand: (overlap structure, gene_df, exon_df)} for the strands that have genes; strand_of: {gene: '+' or '-'}."""
    out = {}
    for s in STRANDS:
        g = gene_df[[strand_of[x] == s for x in gene_df.gene]]
        if len(g):
            out[s] = (get_gene_overlap_structure(g), g, exon_df[exon_df.gene.isin(g.gene)])
    return out


def split_reads(reads_df, sense):
    """{strand: the rows of reads_df of that sense, in order}."""
    sense = np.asarray(sense)
    assert len(sense) == len(reads_df)
    return {s: reads_df[sense == s] for s in STRANDS}


def expected(reads_df, sense, chrom_len, tables, strand, paired):
    """restate on (A^strand, B^strand): (csr, overlap coverage, counts, census)."""
    ov, g, e = tables[strand]
    return ro.restate(split_reads(reads_df, sense)[strand], chrom_len, ov, g, e, paired)


# --- the hand-made case -------------------------------------------------------------------------------------------------

HAND_GENES = [('P', '+', [(101, 300)]),              # P and M share the bases 201 .. 300 on opposite strands
              ('M', '-', [(201, 400)]),
              ('IP', '+', [(1001, 1200)]),           # one isolated gene per strand
              ('IM', '-', [(1501, 1700)]),
              ('A', '+', [(2001, 2300)]),            # a two-gene overlap group on '+'
              ('B', '+', [(2201, 2500)])]
HAND_CHROM_LEN = 3000
# (0-based pos, CIGAR, FLAG): single reads, so the sense is '-' with 0x10 and '+' without
HAND_READS = [(210, '50M', 0),        # r0 shared exon, '+'        unstranded: caught by P and M, dropped
              (220, '50M', 16),       # r1 shared exon, '-'        unstranded: dropped
              (120, '50M', 0),        # r2 P alone, '+'
              (120, '50M', 16),       # r3 P alone, '-'            unstranded: counted for P (antisense)
              (1010, '50M', 0),       # r4 IP, '+'
              (1510, '50M', 16),      # r5 IM, '-'
              (2010, '50M', 0),       # r6 A alone, '+'
              (2210, '50M', 0),       # r7 A and B, '+'            dropped everywhere: same strand
              (2350, '50M', 16),      # r8 B alone, '-'
              (320, '50M', 16)]       # r9 M alone, '-'
HAND_COUNTS = {'no': {'P': 2, 'M': 1, 'IP': 1, 'IM': 1, 'A': 1, 'B': 1},
               'forward': {'P': 2, 'M': 2, 'IP': 1, 'IM': 1, 'A': 1, 'B': 0},
               'reverse': {'P': 2, 'M': 1, 'IP': 0, 'IM': 0, 'A': 0, 'B': 1}}


def hand_case():
    """(reads_df with `flag`, chrom_len, gene_df, exon_df, {gene: strand})."""
    gene_df, exon_df = rf.tables('chrH', [(g, exons) for g, _, exons in HAND_GENES])
    reads = pd.DataFrame([('q{0}'.format(k), p, c, f) for k, (p, c, f) in enumerate(HAND_READS)], columns=['qname', 'pos', 'cigar', 'flag'])
    return reads, HAND_CHROM_LEN, gene_df, exon_df, {g: s for g, s, _ in HAND_GENES}


# --- seeded cases -------------------------------------------------------------------------------------------------------

def stranded_case(seed, paired, n_rows, senses='mixed', one_strand=False):
    """
    A seeded case of n_rows rows: (reads_df, sense array, chrom_len, gene_df, exon_df, {gene: strand}).  The annotation is
    rf.random_layout with a seeded strand per gene (one_strand: every gene on '+', so '-' has none), so genes that overlap
    land on one strand or on two; the reads are the last n_rows of rf.edge_case, where its mutators' rows are (n_rows None:
    all of a case of about 3 000).  senses: 'plus', 'minus' or 'mixed' -- mixed gives the mates of most pairs one sense and
    a seeded fifth of the pairs two.
    """
    reads, layout = rf.edge_case(seed, paired, n=2800 if n_rows is None else 240)
    n_rows = len(reads) if n_rows is None else n_rows
    assert len(reads) >= n_rows
    reads = reads.iloc[len(reads) - n_rows:].reset_index(drop=True)
    chrom, chrom_len, genes = layout
    gene_df, exon_df = rf.tables(chrom, genes)
    rng = np.random.default_rng([seed, 77])
    strand_of = {g: '+' if one_strand or rng.random() < 0.5 else '-' for g, _ in genes}
    if not one_strand:                                              # both strands have genes
        names = [g for g, _ in genes]
        strand_of[names[0]], strand_of[names[-1]] = '+', '-'
    if senses == 'mixed':
        if paired:
            by_pair = {q: STRANDS[int(rng.integers(0, 2))] for q in dict.fromkeys(reads['qname_unpaired'])}
            sense = np.array([by_pair[q] for q in reads['qname_unpaired']], dtype=object)
            flip = rng.random(n_rows) < 0.1                         # one mate of about a fifth of the pairs
            sense[flip] = np.where(sense[flip] == '+', '-', '+')
        else:
            sense = np.array(STRANDS, dtype=object)[rng.integers(0, 2, n_rows)]
    else:
        sense = np.full(n_rows, {'plus': '+', 'minus': '-'}[senses], dtype=object)
    return reads, sense, chrom_len, gene_df, exon_df, strand_of


def two_strand_layout(seed, n_per_strand=30):
    """
    (chrom, chrom_len, genes, {gene: strand}): two seeded rows of genes on one chromosome, p00 ... on '+' and m00 ... on '-',
    each row with genes that overlap, touch or lie apart (as rf.random_layout); the rows know nothing of each other, so genes
    of opposite strands share bases all along.  Genes come in the order of their first base.
    """
    rng = np.random.default_rng([seed, 5])
    genes, strand_of, reach_all = [], {}, 0
    for s, tag in zip(STRANDS, 'pm'):
        reach, prev = 0, None
        for g in range(n_per_strand):
            how = int(rng.integers(0, 10))                          # 0, 1 overlap the gene before; 2 touch it; else apart
            if prev is None:
                start = int(rng.integers(20, 200))
            elif how < 2:
                start = int(rng.integers(max(min(a for a, _ in prev), reach - 100), reach + 1))
            elif how == 2:
                start = reach + 1
            else:
                start = reach + 1 + int(rng.integers(40, 400))
            prev = rf._random_exons(rng, start)
            name = '{0}{1:02d}'.format(tag, g)
            genes.append((name, prev))
            strand_of[name] = s
            reach = max(reach, max(b for _, b in prev))
        reach_all = max(reach_all, reach)
    genes.sort(key=lambda ge: (min(a for a, _ in ge[1]), ge[0]))
    return 'chrS', reach_all + 50, genes, strand_of


def shared_exon_pairs(genes, strand_of):
    """Pairs of genes on opposite strands whose exons share a base."""
    out = []
    for i, (g, ex) in enumerate(genes):
        for h, ex2 in genes[i + 1:]:
            if strand_of[g] != strand_of[h] and any(a <= d and c <= b for a, b in ex for c, d in ex2):
                out.append((g, h))
    return out


def disagreeing_pairs(reads_df, sense):
    """Pair ids with exactly two rows whose senses differ."""
    by = {}
    for q, s in zip(reads_df['qname_unpaired'], sense):
        by.setdefault(q, []).append(s)
    return [q for q, v in by.items() if len(v) == 2 and v[0] != v[1]]


# --- the strand column of the annotation scans ------------------------------------------------------------------------------

STRAND_BYTES = (b'+', b'-', b'.', b'?')


def field7(data, fasta=False):
    """
    Field seven of every exon line of an annotation text (bytes), in file order, as a list of one-byte bytes; fasta: the text
    ends at a line `##FASTA` (GFF3).  A field that is not one of + - . ? raises ValueError((line, 'strand')).  Lines are taken
    as the scans take them: '\\r' before the line end dropped, empty lines and lines that begin with '#' skipped, the third
    field `exon` in any letter case.  The texts this is used on have no other fault.
    """
    out = []
    lines = data.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    for k, ln in enumerate(lines, 1):
        if ln.endswith(b'\r'):
            ln = ln[:-1]
        if fasta and ln.startswith(b'##FASTA'):
            break
        if not ln or ln[:1] == b'#':
            continue
        f = ln.split(b'\t')
        assert len(f) >= 9, k
        if f[2].lower() != b'exon':
            continue
        if f[6] not in STRAND_BYTES:
            raise ValueError((k, 'strand'))
        out.append(f[6])
    return out


def with_field7(data, line, value):
    """The text with field seven of line `line` (1-based) replaced by `value` (bytes)."""
    lines = data.split(b'\n')
    f = lines[line - 1].split(b'\t')
    f[6] = value
    lines[line - 1] = b'\t'.join(f)
    return b'\n'.join(lines)


def exon_lines(data):
    """The 1-based numbers of the exon lines of a text."""
    return [k for k, ln in enumerate(data.split(b'\n'), 1) if ln[:1] not in (b'', b'#') and len(ln.split(b'\t')) >= 9 and ln.split(b'\t')[2].lower() == b'exon']


def first_exons(data, n):
    """The text cut behind its n-th exon line (it has at least n)."""
    at = exon_lines(data)
    assert len(at) >= n
    return b'\n'.join(data.split(b'\n')[:at[n - 1]]) + b'\n'
