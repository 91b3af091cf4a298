"""
GFF3 files for the annotation tests (test tooling, not product code; it shares no code with the product).

`write_twin` writes one seeded annotation twice, as the .gtf `_gtf_fixtures.write_gtf` produces and as a .gff3 in one of three
dialects, so that both loaders must return the same table.  `restate` is a plain Python restatement of the rule in
include/degnorm_amd.h ("GFF3 annotation scan"): the checker of both builds.  `CASES` are small texts that reach every branch
of the rule, `ERRORS` the malformed ones with the line and kind they must give, `mutations` seeded damage of a small file.
`write_pipeline_gff3` is the annotation of the end-to-end fixture in the `ensembl` dialect.
"""
import os

import numpy as np

import _gtf_fixtures as gf

DIALECTS = ('gencode', 'ensembl', 'ncbi')
KINDS = {'fields': 1, 'gene': 2, 'integer': 3, 'parent': 4, 'depth': 5}
TEXT = {'fields': 'must have the 9 mandatory .gff3 columns.\nRead more at https://github.com/The-Sequence-Ontology/Specifications/blob/master/gff3.md',
        'gene': 'is an exon record without a usable gene_name, gene, Parent or gene_id attribute.',
        'integer': 'is an exon record whose start or end is not an integer.',
        'parent': 'is an exon record whose chain of Parent attributes names an ID that no record has.',
        'depth': 'is an exon record whose chain of Parent attributes does not reach a gene within 8 records.'}


def _attrs(pairs):
    return ';'.join('{0}={1}'.format(k, v) for k, v in pairs if v is not None)


def write_twin(directory, seed, min_bytes, dialect):
    """
    The same seeded annotation as <directory>/twin_<dialect>.gtf (written by _gtf_fixtures.write_gtf: min_bytes is the size
    of this one) and as twin_<dialect>.gff3.  Every seventh gene has no name and every eleventh an empty one, as in write_gtf,
    so the gene_id fallback gives the same name in both files.  Returns (gtf path, gff3 path).
      gencode   ID, Parent, gene_id and gene_name on every line
      ensembl   gene lines ID=gene:..;Name=..;gene_id=..; transcripts Parent=gene:..;Name=TX..; exons Parent=transcript:..;Name=ENSE.. only
      ncbi      ID=gene-.., Parent=rna-.., gene=.. on exons, Dbxref=GeneID:1,HGNC:HGNC:2
    """
    gtf, gff3 = os.path.join(directory, 'twin_{0}.gtf'.format(dialect)), os.path.join(directory, 'twin_{0}.gff3'.format(dialect))
    _, n_genes, _ = gf.write_gtf(gtf, seed, min_bytes)
    write_gff3(gff3, seed, n_genes, dialect)
    return gtf, gff3


def write_gff3(gff3, seed, n_genes, dialect):
    """The first n_genes genes of _gtf_fixtures.write_gtf(., seed, .) as a GFF3 file in `dialect`.  Returns (lines, bytes)."""
    assert dialect in DIALECTS
    n_lines = 2
    rng = np.random.default_rng(seed)                 # the draws of write_gtf, gene after gene
    pos = {c: 1000 for c in gf.CHROMS}
    with open(gff3, 'w') as f:
        f.write('##gff-version 3\n#!genome-build none\n')
        for g in range(n_genes):
            chrom = gf.CHROMS[g % len(gf.CHROMS)]
            strand = '+-'[g & 1]
            gid = 'ENSG{0:011d}.{1}'.format(g, 1 + g % 9)
            name = None if g % 7 == 3 else '' if g % 11 == 5 else 'GENE{0}'.format(g)
            n_tx = int(rng.integers(1, 9))
            n_ex = rng.integers(2, 13, size=n_tx)
            ex_len = rng.integers(60, 900, size=int(n_ex.max()))
            gaps = rng.integers(80, 4000, size=int(n_ex.max()))
            start0 = pos[chrom] + int(rng.integers(100, 5000))
            starts = start0 + np.concatenate([[0], np.cumsum(ex_len[:-1] + gaps[:-1])])
            ends = starts + ex_len - 1
            pos[chrom] = int(ends[-1])
            row = '{0}\tHAVANA\t{1}\t{2}\t{3}\t.\t{4}\t{5}\t{6}\n'
            if dialect == 'gencode':
                common = [('gene_id', gid), ('gene_type', 'protein_coding'), ('gene_name', name), ('level', 2)]
                out = [row.format(chrom, 'gene', starts[0], ends[-1], strand, '.', _attrs([('ID', gid)] + common))]
            elif dialect == 'ensembl':
                out = [row.format(chrom, 'gene', starts[0], ends[-1], strand, '.',
                                  _attrs([('ID', 'gene:' + gid), ('Name', name), ('biotype', 'protein_coding'), ('gene_id', gid), ('version', 1)]))]
            else:
                out = [row.format(chrom, 'gene', starts[0], ends[-1], strand, '.',
                                  _attrs([('ID', 'gene-' + gid), ('Dbxref', 'GeneID:1,HGNC:HGNC:2'), ('Name', name), ('gbkey', 'Gene'), ('gene', name),
                                          ('gene_id', gid if not name else None)]))]
            for t in range(n_tx):
                k = int(n_ex[t])
                tid = 'ENST{0:011d}.{1}'.format(g * 8 + t, 1 + t)
                if dialect == 'gencode':
                    tx = [('Parent', gid), ('gene_id', gid), ('transcript_id', tid), ('gene_name', name), ('transcript_name', 'TX{0}-20{1}'.format(g, t)),
                          ('tag', 'basic,CCDS')]
                    out.append(row.format(chrom, 'transcript', starts[0], ends[k - 1], strand, '.', _attrs([('ID', tid)] + tx)))
                elif dialect == 'ensembl':
                    out.append(row.format(chrom, 'mRNA', starts[0], ends[k - 1], strand, '.',
                                          _attrs([('ID', 'transcript:' + tid), ('Parent', 'gene:' + gid), ('Name', 'TX{0}-20{1}'.format(g, t)),
                                                  ('biotype', 'protein_coding'), ('transcript_id', tid)])))
                else:
                    out.append(row.format(chrom, 'mRNA', starts[0], ends[k - 1], strand, '.',
                                          _attrs([('ID', 'rna-' + tid), ('Parent', 'gene-' + gid), ('Dbxref', 'GeneID:1,HGNC:HGNC:2'),
                                                  ('Name', tid), ('gbkey', 'mRNA'), ('gene', name), ('product', 'protein%2C isoform {0}'.format(t))])))
                for e in range(k):
                    ense = 'ENSE{0:011d}.1'.format((g * 8 + t) * 12 + e)
                    a, b = starts[e], ends[e]
                    if dialect == 'gencode':
                        ex = [('ID', 'exon:{0}:{1}'.format(tid, e + 1))] + [('Parent', tid)] + tx[1:] + [('exon_number', e + 1), ('exon_id', ense)]
                        cds = [('ID', 'CDS:' + tid)] + ex[1:]
                    elif dialect == 'ensembl':
                        ex = [('Parent', 'transcript:' + tid), ('Name', ense), ('constitutive', 0), ('exon_id', ense), ('rank', e + 1)]
                        cds = [('ID', 'CDS:ENSP' + tid[4:]), ('Parent', 'transcript:' + tid), ('protein_id', 'ENSP' + tid[4:])]
                    else:
                        ex = [('ID', 'exon-{0}-{1}'.format(tid, e + 1)), ('Parent', 'rna-' + tid), ('Dbxref', 'GeneID:1,HGNC:HGNC:2'), ('gbkey', 'mRNA'),
                              ('gene', name), ('product', 'protein%2C isoform {0}'.format(t))]
                        cds = [('ID', 'cds-' + tid), ('Parent', 'rna-' + tid), ('Dbxref', 'GeneID:1,HGNC:HGNC:2'), ('gbkey', 'CDS'), ('gene', name)]
                    out.append(row.format(chrom, 'exon', a, b, strand, '.', _attrs(ex)))
                    out.append(row.format(chrom, 'CDS', a, b, strand, e % 3, _attrs(cds)))
            out.append('###\n')
            f.write(''.join(out))
            n_lines += len(out)
    return n_lines, os.path.getsize(gff3)


# --- the rule, restated ---------------------------------------------------------------------------------------------------

def _tags(field):
    """{tag: value} of an attribute field: the first piece with a tag wins; Parent cut to its first element."""
    tags = {}
    for piece in field.split(b';'):
        tag, _, value = piece.strip(b' ').partition(b'=')
        tags.setdefault(tag.strip(b' '), value.strip(b' '))
    if b'Parent' in tags:
        tags[b'Parent'] = tags[b'Parent'].split(b',')[0].strip(b' ')
    return tags


def _first(tags, names):
    for k in names:
        if tags.get(k):
            return tags[k]
    return None


def restate(data, hash_bits=64):
    """
    The rule on the bytes of a GFF3 file, line by line with dicts: (number of lines, line numbers, chr, start, end, gene of
    the exon lines in file order -- names as lists of bytes).  Malformed input: ValueError((line, kind)).  hash_bits is taken
    for symmetry with gff3_scan: nothing here hashes, which is the point.
    """
    lines = data.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    nodes, exons = {}, []
    for k, ln in enumerate(lines, 1):
        if ln.endswith(b'\r'):
            ln = ln[:-1]
        if ln == b'##FASTA':
            break
        if not ln or ln[:1] == b'#':
            continue
        f = ln.split(b'\t')
        if len(f) < 9:
            raise ValueError((k, 'fields'))
        tags = _tags(f[8])
        if f[2].lower() == b'exon':
            if not (f[3].isdigit() and f[4].isdigit() and len(f[3]) <= 18 and len(f[4]) <= 18 and f[3].isascii() and f[4].isascii()):
                raise ValueError((k, 'integer'))
            own = _first(tags, (b'gene_name', b'gene'))
            if own is None and not tags.get(b'Parent'):
                own = _first(tags, (b'gene_id',))
                if own is None:
                    raise ValueError((k, 'gene'))
            exons.append((k, f[0], int(f[3]), int(f[4]), own, tags.get(b'Parent')))
        elif tags.get(b'ID'):
            nodes.setdefault(tags[b'ID'], (tags.get(b'Parent') or None, _first(tags, (b'gene_name', b'gene')), _first(tags, (b'Name', b'gene_id', b'ID'))))
    no, chrs, starts, ends, genes = [], [], [], [], []
    for k, chrom, a, b, own, parent in exons:
        if own is None:
            want = parent
            for _ in range(8):
                if want not in nodes:
                    raise ValueError((k, 'parent'))
                up, gname, rname = nodes[want]
                if gname is not None:
                    own = gname
                elif up is None:
                    own = rname
                else:
                    want = up
                    continue
                break
            else:
                raise ValueError((k, 'depth'))
        no.append(k); chrs.append(chrom); starts.append(a); ends.append(b); genes.append(own)
    return len(lines), no, chrs, starts, ends, genes


# --- small texts ----------------------------------------------------------------------------------------------------------

def _ln(chrom, kind, a, b, attrs):
    return '{0}\tsrc\t{1}\t{2}\t{3}\t.\t+\t.\t{4}'.format(chrom, kind, a, b, attrs).encode()


def _chain(n):
    """An exon under n nested nodes, of which only the top one can name it: n lookups.  Children stand before parents."""
    out = [_ln('c1', 'exon', 10, 20, 'Parent=n1')]
    for k in range(1, n):
        out.append(_ln('c1', 'region', 1, 100, 'ID=n{0};Parent=n{1}'.format(k, k + 1)))
    out.append(_ln('c1', 'gene', 1, 100, 'ID=n{0};Name=TOP'.format(n)))
    return b'\n'.join(out) + b'\n'


_GENE = _ln('c1', 'gene', 1, 500, 'ID=gene:G1;Name=ALPHA;gene_id=G1')
_TX = _ln('c1', 'mRNA', 1, 500, 'ID=transcript:T1;Parent=gene:G1;Name=ALPHA-201')
_EX = _ln('c1', 'exon', 10, 90, 'Parent=transcript:T1;Name=E1')
_OWN = _ln('c2', 'exon', 5, 50, 'ID=e9;gene_name=OWN')
_LONG = _ln('c1', 'mRNA', 1, 500, 'ID=transcript:T2;Parent=gene:G1;Note=' + 'x' * 6000)

CASES = {
    'one_line': _OWN,
    'one_line_newline': _OWN + b'\n',
    'ensembl_small': b'\n'.join([b'##gff-version 3', _GENE, _TX, _EX, b'###', _ln('c1', 'EXON', 100, 190, 'Parent=transcript:T1')]) + b'\n',
    'no_final_newline': b'\n'.join([_GENE, _TX, _EX]),
    'headers_blank_crlf': b'\r\n'.join([b'##gff-version 3', b'', b'#!x', _GENE, b'', _TX, b'###', _EX, b'', _OWN]) + b'\r\n',
    'fasta_tail': b'\n'.join([_GENE, _TX, _EX, b'##FASTA', b'>c1', b'ACGT\tACGT', b'c1\tx\texon\tq\t2\t.\t+\t.\tgene=Z', _ln('c1', 'exon', 1, 2, 'Parent=nobody'),
                              _ln('c1', 'exon', 3, 4, 'gene=LATE'), b'ACGTACGT']) + b'\n',
    'fasta_crlf_first': b'##FASTA\r\n>c1\r\nACGT\r\n',
    'not_quite_fasta': b'\n'.join([b'##FASTA ', b'##fasta', b'###FASTA', _OWN]) + b'\n',
    'children_first': b'\n'.join([_EX, _ln('c1', 'exon', 100, 190, 'Parent=transcript:T1'), _TX, _GENE]) + b'\n',
    'several_parents': b'\n'.join([_GENE, _TX, _ln('c1', 'gene', 1, 9, 'ID=gene:G2;Name=BETA'), _ln('c1', 'mRNA', 1, 9, 'ID=transcript:T9;Parent=gene:G2'),
                                   _ln('c1', 'exon', 10, 90, 'Parent=transcript:T9,transcript:T1'), _ln('c1', 'exon', 10, 91, 'Parent= transcript:T1 , transcript:T9'),
                                   _ln('c1', 'exon', 10, 92, 'Parent=,transcript:T1;gene_id=FALLBACK')]) + b'\n',
    'repeated_ids': b'\n'.join([_ln('c1', 'CDS', 1, 9, 'ID=dup;Name=FIRST'), _ln('c1', 'CDS', 20, 29, 'ID=dup;Name=SECOND'), _ln('c1', 'exon', 1, 9, 'Parent=dup'),
                                _ln('c1', 'CDS', 40, 49, 'ID=dup;gene=THIRD')]) + b'\n',
    'spaces': b'\n'.join([_ln('c1', 'gene', 1, 9, ' ID = g 1 ; Name =  SPACED NAME  ;'), _ln('c1', 'exon', 1, 9, ' Parent = g 1 ;; x'),
                          _ln('c1', 'exon', 2, 9, 'note=a=b; gene_name = A=B ')]) + b'\n',
    'empty_values': b'\n'.join([_ln('c1', 'gene', 1, 9, 'ID=g1;gene_name=;gene=;Name=;gene_id=GID'), _ln('c1', 'exon', 1, 9, 'gene_name=;gene=;Parent=g1'),
                                _ln('c1', 'gene', 1, 9, 'ID=g2;Name=;gene_id='), _ln('c1', 'exon', 2, 9, 'gene_name;Parent=g2'),
                                _ln('c1', 'exon', 3, 9, 'gene_name=;gene_name=SECOND;gene_id=THIRD'), _ln('c1', 'gene', 1, 9, 'ID=;Name=NOID'),
                                _ln('c1', 'exon', 4, 9, 'Parent=;gene_id=X')]) + b'\n',
    'gene_against_gene_id': b'\n'.join([_ln('c1', 'exon', 1, 9, 'gene_id=ID1;Gene=no;GENE=no;gene_names=no;gene=YES'), _ln('c1', 'exon', 2, 9, 'gene_id=ID2;xgene=no'),
                                        _ln('c1', 'gene', 1, 9, 'ID=g;gene_id=GID;name=no;Name=RN'), _ln('c1', 'exon', 3, 9, 'gene_id=ID3;Parent=g;parent=no;id=no')]) + b'\n',
    'exon_with_id_is_no_node': b'\n'.join([_ln('c1', 'exon', 1, 9, 'ID=e1;gene=A'), _ln('c1', 'gene', 1, 9, 'ID=e2;Name=B'), _ln('c1', 'exon', 2, 9, 'Parent=e2')]) + b'\n',
    'chain_8': _chain(8),
    'tenth_field': _ln('c1', 'gene', 1, 9, 'ID=g;Name=N\tgene=EXTRA') + b'\n' + _ln('c1', 'exon', 1, 9, 'Parent=g\tgene=EXTRA\tmore') + b'\n',
    'gname_midway': b'\n'.join([_ln('c1', 'gene', 1, 9, 'ID=g;Name=TOP'), _ln('c1', 'mRNA', 1, 9, 'ID=t;Parent=g;gene=MID;Name=TN'), _ln('c1', 'exon', 1, 9, 'Parent=t')]) + b'\n',
    'long_line': b'\n'.join([_GENE, _LONG, _ln('c1', 'exon', 10, 90, 'Parent=transcript:T2'), _TX, _EX]) + b'\n',
    'many_lines': b'\n'.join(_ln('c{0}'.format(k % 3), 'exon' if k % 3 else 'gene', k + 1, k + 9,
                                 'ID=n{0};Name=N{0}'.format(k) if k % 3 == 0 else 'Parent=n{0}'.format(k - k % 3 if k % 5 else (k - k % 3 + 300) % 780))
                             for k in range(780)) + b'\n',              # more than one 256-line block; every fifth exon names a node far ahead or behind
    'big_integers': _ln('c1', 'exon', '0' * 17 + '7', '9' * 18, 'gene=G') + b'\n',
}

ERRORS = {
    'few_fields': (b'\n'.join([_GENE, b'c1\tsrc\texon\t1\t2\t.\t+\t.']) + b'\n', 2, 'fields'),
    'no_tabs': (b'just words', 1, 'fields'),
    'bad_start': (b'\n'.join([_GENE, _TX, _ln('c1', 'exon', '1x', 9, 'gene=G')]) + b'\n', 3, 'integer'),
    'empty_end': (_ln('c1', 'exon', 1, '', 'gene=G') + b'\n', 1, 'integer'),
    'long_integer': (_ln('c1', 'exon', 1, '1' * 19, 'gene=G'), 1, 'integer'),
    'integer_before_gene': (_ln('c1', 'exon', -1, 5, 'x=y') + b'\n', 1, 'integer'),
    'nothing_usable': (b'\n'.join([_GENE, _ln('c1', 'exon', 1, 9, 'ID=e1;Name=E;gene_name=;gene_id=;Parent=')]) + b'\n', 2, 'gene'),
    'empty_attributes': (_ln('c1', 'exon', 1, 9, ''), 1, 'gene'),
    'dangling_parent': (b'\n'.join([_GENE, _TX, _EX, _ln('c1', 'exon', 1, 9, 'Parent=transcript:T')]) + b'\n', 4, 'parent'),
    'dangling_grandparent': (b'\n'.join([_TX, _EX]) + b'\n', 2, 'parent'),
    'no_nodes_at_all': (_EX + b'\n', 1, 'parent'),
    'parent_is_an_exon': (b'\n'.join([_ln('c1', 'exon', 1, 9, 'ID=e1;gene=A'), _ln('c1', 'exon', 2, 9, 'Parent=e1')]) + b'\n', 2, 'parent'),
    'chain_9': (_chain(9), 1, 'depth'),
    'cycle_of_two': (b'\n'.join([_ln('c1', 'mRNA', 1, 9, 'ID=a;Parent=b'), _ln('c1', 'mRNA', 1, 9, 'ID=b;Parent=a'), _OWN, _ln('c1', 'exon', 1, 9, 'Parent=a')]) + b'\n', 4, 'depth'),
    'self_parent': (b'\n'.join([_ln('c1', 'mRNA', 1, 9, 'ID=a;Parent=a'), _ln('c1', 'exon', 1, 9, 'Parent=a')]) + b'\n', 2, 'depth'),
    'first_link_error_wins': (b'\n'.join([_ln('c1', 'mRNA', 1, 9, 'ID=a;Parent=a'), _OWN, _ln('c1', 'exon', 1, 9, 'Parent=a'), _ln('c1', 'exon', 1, 9, 'Parent=zz')]) + b'\n', 3, 'depth'),
    'line_error_wins_over_link_error': (b'\n'.join([_GENE, _TX, _ln('c1', 'exon', 1, 9, 'Parent=nobody')] + [_EX] * 86 + [b'c1\tsrc\tgene\t1']) + b'\n', 90, 'fields'),
    'first_line_error_wins': (b'\n'.join([_GENE, _ln('c1', 'exon', 1, 9, 'x=y'), b'oops', _ln('c1', 'exon', 'a', 9, 'gene=G')]) + b'\n', 2, 'gene'),
    'error_before_fasta': (b'\n'.join([_GENE, b'oops', b'##FASTA', b'>c1']) + b'\n', 2, 'fields'),
    'link_error_before_fasta': (b'\n'.join([_EX, b'##FASTA', _TX, _GENE]) + b'\n', 1, 'parent'),
}


def small_file():
    """A 40-line file with every kind of line, for the mutations."""
    out = [b'##gff-version 3']
    for g in range(6):
        out.append(_ln('c1', 'gene', 100 * g + 1, 100 * g + 90, 'ID=gene:G{0};Name=NAME{0};gene_id=G{0}'.format(g)))
        out.append(_ln('c1', 'mRNA', 100 * g + 1, 100 * g + 90, 'ID=transcript:T{0};Parent=gene:G{0}'.format(g)))
        for e in range(2):
            out.append(_ln('c1', 'exon', 100 * g + 10 * e + 1, 100 * g + 10 * e + 9, 'Parent=transcript:T{0};Name=E{0}{1}'.format(g, e)))
        out.append(_ln('c1', 'CDS', 100 * g + 1, 100 * g + 9, 'ID=cds{0};Parent=transcript:T{0}'.format(g)))
        out.append(_ln('c2', 'exon', 100 * g + 1, 100 * g + 9, 'ID=x{0};gene=OWN{0}'.format(g)) if g % 2 else b'###')
    return b'\n'.join(out) + b'\n'


def mutations(n, seed=5):
    """n seeded mutations of small_file(): a byte replaced (often by a byte that matters to the rule), or a line cut."""
    rng = np.random.default_rng(seed)
    base = small_file()
    special = b'\t\n\r;=, #:0eEPI\x00\xff'
    for _ in range(n):
        data = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            what = int(rng.integers(0, 4))
            p = int(rng.integers(0, len(data)))
            if what == 0:
                data[p] = int(rng.integers(0, 256))
            elif what in (1, 2):
                data[p] = special[int(rng.integers(0, len(special)))]
            else:
                q = data.find(b'\n', p)
                del data[p:(q if q >= 0 else len(data))]
        if data:
            yield bytes(data)


def outcome(fn, data, **kw):
    """fn's result on data as comparable values: ('rows', lines, rows) or ('error', line, kind)."""
    try:
        n_lines, no, chrs, starts, ends, genes = fn(data, **kw)
    except ValueError as e:
        return ('error',) + tuple(e.args[0])
    return ('rows', n_lines, list(zip(no, chrs, starts, ends, genes)))


def write_pipeline_gff3(path):
    """_gtf_fixtures.pipeline_layouts() in the ensembl dialect: the genes of write_pipeline_gtf, with exons that name only their transcript."""
    layouts = gf.pipeline_layouts()
    rows = []
    for k in range(max(len(genes) for _, _, genes in layouts)):
        for chrom, _, genes in layouts:
            if k < len(genes):
                rows.append((chrom,) + genes[k])
    with open(path, 'w') as f:
        f.write('##gff-version 3\n')
        for chrom, g, exons in rows:
            lo, hi = min(a for a, _ in exons), max(b for _, b in exons)
            row = '{0}\ttest\t{1}\t{2}\t{3}\t.\t+\t{4}\t{5}\n'
            for j, (a, b) in enumerate(exons[:1]):           # one exon stands before its parents
                f.write(row.format(chrom, 'exon', a, b, '.', 'Parent=transcript:T_{0};Name=E_{0}_{1};rank={1}'.format(g, j + 1)))
            f.write(row.format(chrom, 'gene', lo, hi, '.', 'ID=gene:ID_{0};Name={0};biotype=protein_coding;gene_id=ID_{0}'.format(g)))
            f.write(row.format(chrom, 'mRNA', lo, hi, '.', 'ID=transcript:T_{0};Parent=gene:ID_{0};Name={0}-201'.format(g)))
            for j, (a, b) in enumerate(exons):
                if j > 0:
                    f.write(row.format(chrom, 'exon', a, b, '.', 'Parent=transcript:T_{0};Name=E_{0}_{1};rank={1}'.format(g, j + 1)))
                f.write(row.format(chrom, 'CDS', a, b, 0, 'ID=CDS:P_{0};Parent=transcript:T_{0}'.format(g)))
            f.write('###\n')
