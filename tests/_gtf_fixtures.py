"""
GTF files for the annotation and pipeline tests (test tooling, not product code).

`write_gtf` writes a seeded GENCODE-style annotation of any size; `restate` is a plain Python restatement of the scanner's
rule (include/degnorm_amd.h, dn_gtf_scan) that shares no code with the product: the checker of the test at size.
`with_noise` rewrites a GTF with `#` header lines, interleaved blank lines and \\r\\n line ends.  The `pipeline_*` functions
are the annotation, BAM references and seeded reads of the end-to-end fixture (tests/golden/make_golden_pipeline.py runs
the reference on them).
"""
import numpy as np
import pandas as pd

import _reads_fixtures as rf

CHROMS = ['chr1', 'chr2', 'chr10', 'chrX', 'chrUn_gl000220', '3']


def write_gtf(path, seed, min_bytes, header=True):
    """
    A seeded annotation of at least min_bytes: per gene a `gene` line and 1-8 transcripts, each a `transcript` line and 2-12
    exons with `exon` and `CDS` lines (about 280 bytes a line, GENCODE-style attributes, gene_id before gene_name; every
    seventh gene has no gene_name, every eleventh an empty one).  Returns (lines, genes, bytes).
    """
    rng = np.random.default_rng(seed)
    n_lines, n_genes, size = 0, 0, 0
    with open(path, 'w') as f:
        if header:
            head = '##description: seeded test annotation\n##provider: tests\n#!genome-build none\n'
            f.write(head)
            size += len(head)
            n_lines += 3
        pos = {c: 1000 for c in CHROMS}
        while size < min_bytes:
            g = n_genes
            n_genes += 1
            chrom = CHROMS[g % len(CHROMS)]
            strand = '+-'[g & 1]
            gid = 'ENSG{0:011d}.{1}'.format(g, 1 + g % 9)
            name = '' if g % 7 == 3 else ' gene_name "{0}";'.format('' if g % 11 == 5 else 'GENE{0}'.format(g))
            n_tx = int(rng.integers(1, 9))
            n_ex = rng.integers(2, 13, size=n_tx)
            ex_len = rng.integers(60, 900, size=int(n_ex.max()))
            gaps = rng.integers(80, 4000, size=int(n_ex.max()))
            start0 = pos[chrom] + int(rng.integers(100, 5000))
            starts = start0 + np.concatenate([[0], np.cumsum(ex_len[:-1] + gaps[:-1])])
            ends = starts + ex_len - 1
            pos[chrom] = int(ends[-1])
            gattr = 'gene_id "{0}"; gene_type "protein_coding";{1} level 2; tag "overlapping_locus";'.format(gid, name)
            out = ['{0}\tHAVANA\tgene\t{1}\t{2}\t.\t{3}\t.\t{4}\n'.format(chrom, starts[0], ends[-1], strand, gattr)]
            for t in range(n_tx):
                k = int(n_ex[t])
                tid = 'ENST{0:011d}.{1}'.format(g * 8 + t, 1 + t)
                tattr = ('gene_id "{0}"; transcript_id "{1}"; gene_type "protein_coding";{2} transcript_type "protein_coding"; '
                         'transcript_name "TX{3}-20{4}"; level 2; transcript_support_level "1"; tag "basic"; tag "CCDS"; '
                         'havana_gene "OTTHUMG{5:011d}.2";').format(gid, tid, name, g, t, g)
                out.append('{0}\tHAVANA\ttranscript\t{1}\t{2}\t.\t{3}\t.\t{4}\n'.format(chrom, starts[0], ends[k - 1], strand, tattr))
                for e in range(k):
                    tail = ' exon_number {0}; exon_id "ENSE{1:011d}.1";'.format(e + 1, (g * 8 + t) * 12 + e)
                    a, b = starts[e], ends[e]
                    out.append('{0}\tHAVANA\texon\t{1}\t{2}\t.\t{3}\t.\t{4}{5}\n'.format(chrom, a, b, strand, tattr, tail))
                    out.append('{0}\tHAVANA\tCDS\t{1}\t{2}\t.\t{3}\t{4}\t{5}{6}\n'.format(chrom, a, b, strand, e % 3, tattr, tail))
            text = ''.join(out)
            f.write(text)
            size += len(text)
            n_lines += len(out)
    return n_lines, n_genes, size


def gene_of(attribute):
    """The gene name of an attribute field (bytes), or None: the reference's _attribute_to_gene, restated."""
    pieces = [x.strip(b' ') for x in attribute.split(b';')]
    for tag in (b'gene_name', b'gene_id'):
        hits = [x for x in pieces if x.startswith(tag)]
        if hits:
            value = hits[0][len(tag):].strip(b' "')
            if value:
                return value
    return None


def restate(data):
    """
    The scanner's rule on the bytes of a GTF file, line by line: (number of lines, line numbers, chr, start, end, gene of
    the exon lines in file order -- names as lists of bytes).  Malformed input: ValueError((line, kind)).
    """
    lines = data.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    no, chrs, starts, ends, genes = [], [], [], [], []
    for k, ln in enumerate(lines, 1):
        if ln.endswith(b'\r'):
            ln = ln[:-1]
        if not ln or ln[:1] == b'#':
            continue
        f = ln.split(b'\t')
        if len(f) < 9:
            raise ValueError((k, 'fields'))
        if f[2].lower() != b'exon':
            continue
        if not (f[3].isdigit() and f[4].isdigit() and len(f[3]) <= 18 and len(f[4]) <= 18):
            raise ValueError((k, 'integer'))
        g = gene_of(f[8])
        if g is None:
            raise ValueError((k, 'gene'))
        no.append(k); chrs.append(f[0]); starts.append(int(f[3])); ends.append(int(f[4])); genes.append(g)
    return len(lines), no, chrs, starts, ends, genes


def with_noise(src, dst, crlf=True):
    """src rewritten with three `#` header lines, a blank line after every fifth line and (crlf) \\r\\n line ends."""
    with open(src, 'rb') as f:
        data = f.read()
    nl = b'\r\n' if crlf else b'\n'
    lines = data.split(b'\n')
    last_open = lines[-1] != b''                 # the source does not end in a newline: neither does the copy
    if not last_open:
        lines.pop()
    out = [b'##gff-version 2', b'#!genome-build test', b'# exon gene_name "not a record"']
    for k, ln in enumerate(lines):
        out.append(ln)
        if k % 5 == 4:
            out.append(b'')
    with open(dst, 'wb') as f:
        f.write(nl.join(out) + (b'' if last_open else nl))


# --- the end-to-end fixture ------------------------------------------------------------------------------------------------

PIPELINE_REFS = [('chr1', 6000), ('chr2', 2000), ('chrM', 500)]          # chrM: a BAM reference the annotation lacks
PIPELINE_SAMPLES = ['s1', 's2', 's3']


def pipeline_layouts():
    """The annotated chromosomes: the golden and quiet layouts of _reads_fixtures and one no BAM file has."""
    return [rf.golden_layout(), rf.quiet_layout(), ('chr7', 3000, [('Z', [(101, 400), (601, 800)])])]


def write_pipeline_gtf(path):
    """pipeline.gtf: a gene line per gene, an exon and a CDS line per exon, chromosomes interleaved gene by gene."""
    layouts = pipeline_layouts()
    rows = []
    for k in range(max(len(genes) for _, _, genes in layouts)):
        for chrom, _, genes in layouts:
            if k < len(genes):
                rows.append((chrom,) + genes[k])
    with open(path, 'w') as f:
        for chrom, g, exons in rows:
            attr = 'gene_id "ID_{0}"; gene_name "{0}";'.format(g)
            f.write('{0}\ttest\tgene\t{1}\t{2}\t.\t+\t.\t{3}\n'.format(chrom, min(a for a, _ in exons), max(b for _, b in exons), attr))
            for j, (a, b) in enumerate(exons):
                f.write('{0}\ttest\texon\t{1}\t{2}\t.\t+\t.\t{3} exon_number {4};\n'.format(chrom, a, b, attr, j + 1))
                f.write('{0}\ttest\tCDS\t{1}\t{2}\t.\t+\t0\t{3} exon_number {4};\n'.format(chrom, a, b, attr, j + 1))


def pipeline_reads(sample):
    """{chromosome: reads DataFrame (qname, pos, cigar)} of sample 0, 1 or 2: seeds 10-12 on chr1, 20-22 on chr2."""
    return {'chr1': rf.synth_reads(10 + sample, rf.golden_layout(), 1500),
            'chr2': rf.synth_reads(20 + sample, rf.quiet_layout(), 400, skip=('R',), noise=0.0)}


def pipeline_bam_rows(sample):
    """The sample's reads as the rows _bam_fixtures.write_bam takes (PIPELINE_REFS order), plus two reads on chrM."""
    parts = []
    for tid, (name, _) in enumerate(PIPELINE_REFS[:2]):
        r = pipeline_reads(sample)[name]
        parts.append(pd.DataFrame({'ref': tid, 'pos': r.pos.values, 'qname': [name + q for q in r.qname], 'cigar': r.cigar.values,
                                   'nh': 1, 'nh_type': 'C'}))
    parts.append(pd.DataFrame({'ref': 2, 'pos': [10, 40], 'qname': ['m0', 'm1'], 'cigar': ['30M', '25M'], 'nh': 1, 'nh_type': 'C'}))
    return pd.concat(parts, ignore_index=True)
