"""
GPU tests of the strand column of the two annotation scans (dn_gtf_scan_strand, dn_gff3_window_strand; k_strand_check and
k_row_strand, csrc/dn_annot.hpp): field seven of every exon line, read from the line itself.

  the column equals the restatement (tests/_strand_cases.field7) and, for GFF3, the host build's, on the GTF fixture and the
  three GFF3 dialects at about 200 KB, scanned in 4 KiB windows and in one window
  texts of exactly 1, 255, 256 and 257 exon lines: the parse kernels' block size and its neighbours
  malformed fields (x, empty, ++) raise the ValueError texts of the host build, with file and line, under the first-error rule,
  and only when the strand is asked for
  get_data() without `strand` returns the tables it returned before, on the same files
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gff3_fixtures as g3                                     # noqa: E402
import _gtf_fixtures as gf                                      # noqa: E402
import _strand_cases as sc                                      # noqa: E402
from degnorm_amd import loaders                                 # noqa: E402
from degnorm_amd.gene_processing import GeneAnnotationProcessor  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = 500_000                                              # of the GTF twin; the GFF3 forms of it are about 200 KB
BAD_FIELDS = (b'x', b'', b'++')
LINE_COUNTS = (1, 255, 256, 257)
STRAND_TEXT = 'is an exon record whose strand (column 7) is not one of + - . ?'


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """{'gtf' | dialect: (path, bytes)} of one seeded annotation of about 200 KB in the four forms."""
    d = str(tmp_path_factory.mktemp('strand_annotation'))
    out = {}
    for dialect in g3.DIALECTS:
        gtf, gff3 = g3.write_twin(d, 11, SIZE, dialect)
        out[dialect] = gff3
    out['gtf'] = gtf
    return {k: (p, open(p, 'rb').read()) for k, p in out.items()}


def _loader(path, **kw):
    return loaders.annotation_loader(path, **kw)


@pytest.mark.parametrize('form', ('gtf',) + g3.DIALECTS)
def test_strand_column_equals_restatement_in_small_windows_and_in_one(form, files):
    path, data = files[form]
    want = b''.join(sc.field7(data, fasta=form != 'gtf'))
    assert len(want) > 300 and set(want) == set(b'+-')
    tables = {}
    for window in (4096, None):
        ld = _loader(path, window_bytes=window)
        codes = ld.exon_codes(strand=True)
        assert codes[6].dtype == np.uint8 and codes[6].tobytes() == want, window
        plain = _loader(path, window_bytes=window).exon_codes()
        assert len(plain) == 6 and all(np.array_equal(a, b) for a, b in zip(codes[:4], plain[:4])) and codes[4:6] == plain[4:6]
        tables[window] = _loader(path, window_bytes=window).get_data(strand=True)
    pd.testing.assert_frame_equal(tables[4096], tables[None])
    # get_data() without the argument: the table it was, column for column
    table = _loader(path).get_data()
    assert list(table.columns) == ['chr', 'start', 'end', 'gene']
    assert list(tables[None].columns) == ['chr', 'start', 'end', 'gene', 'strand']
    pd.testing.assert_frame_equal(tables[None].drop(columns='strand'), table)
    assert set(tables[None].strand) == {'+', '-'}
    if form != 'gtf':                                           # the host build of the same source
        n, cols, err = loaders.gff3_scan(data, strand=True)
        assert err is None and cols['strand'].tobytes() == want
        n, dev, err = loaders.gff3_scan(data, device=0, strand=True)
        assert err is None and all(dev[k].tobytes() == cols[k].tobytes() for k in cols)


@pytest.mark.parametrize('n_exons', LINE_COUNTS)
@pytest.mark.parametrize('form', ['gtf', 'ensembl'])
def test_texts_around_the_block_size(form, n_exons, files, tmp_path):
    text = sc.first_exons(files[form][1], n_exons)
    marks = b'+-.?'
    at = sc.exon_lines(text)
    assert len(at) == n_exons
    for k in (0, n_exons // 2, n_exons - 1):                    # the first, a middle and the last row carry . ? and the like
        text = sc.with_field7(text, at[k], marks[(k + 2) % 4:(k + 2) % 4 + 1])
    want = b''.join(sc.field7(text, fasta=form != 'gtf'))
    assert len(want) == n_exons
    p = str(tmp_path / ('t.gtf' if form == 'gtf' else 't.gff3'))
    with open(p, 'wb') as f:
        f.write(text)
    assert _loader(p).exon_codes(strand=True)[6].tobytes() == want
    assert _loader(p, window_bytes=1000).exon_codes(strand=True)[6].tobytes() == want
    if form != 'gtf':
        assert loaders.gff3_scan(text, device=0, strand=True)[1]['strand'].tobytes() == want
    # the last line without its newline
    with open(p, 'wb') as f:
        f.write(text[:-1])
    assert _loader(p).exon_codes(strand=True)[6].tobytes() == want


@pytest.mark.parametrize('bad', BAD_FIELDS)
@pytest.mark.parametrize('form', ['gtf', 'ensembl', 'ncbi'])
def test_malformed_strand_fields(form, bad, files, tmp_path):
    path, data = files[form]
    at = sc.exon_lines(data)
    p = str(tmp_path / ('m.gtf' if form == 'gtf' else 'm.gff3'))
    clean = _loader(path).get_data()
    for line in (at[0], at[255], at[256], at[-1]):
        text = sc.with_field7(data, line, bad)
        with open(p, 'wb') as f:
            f.write(text)
        for window in (4096, None):
            with pytest.raises(ValueError) as e:
                _loader(p, window_bytes=window).get_data(strand=True)
            assert str(e.value) == 'File {0}, line {1} {2}'.format(p, line, STRAND_TEXT)
        if form != 'gtf':                                       # the host build's error, line and kind
            assert loaders.gff3_scan(text, strand=True)[2] == (line, 6) == loaders.gff3_scan(text, device=0, strand=True)[2]
        pd.testing.assert_frame_equal(_loader(p).get_data(), clean)        # not asked for: loads as today
    # the first faulty line wins, whatever its fault
    lines = data.split(b'\n')
    short = b'chr1\tx\texon\t1'
    text = sc.with_field7(b'\n'.join(lines[:at[300] - 1] + [short] + lines[at[300] - 1:]), at[100], bad)
    with open(p, 'wb') as f:
        f.write(text)
    for window in (4096, None):
        with pytest.raises(ValueError, match='line {0} is an exon record whose strand'.format(at[100])):
            _loader(p, window_bytes=window).get_data(strand=True)
    text = sc.with_field7(b'\n'.join(lines[:at[50] - 1] + [short] + lines[at[50] - 1:]), at[100] + 1, bad)
    with open(p, 'wb') as f:
        f.write(text)
    for window in (4096, None):
        with pytest.raises(ValueError, match='line {0} must have the 9 mandatory'.format(at[50])):
            _loader(p, window_bytes=window).get_data(strand=True)


@pytest.mark.parametrize('form', ['gtf', 'gencode'])
def test_processor_keeps_the_column_and_applies_the_gene_rule(form, files, tmp_path):
    path, data = files[form]
    plain = GeneAnnotationProcessor(path, verbose=False).run()
    proc = GeneAnnotationProcessor(path, verbose=False, strand=True)
    out = proc.run()
    assert proc.unstranded_genes == [] and list(out.columns) == ['chr', 'start', 'end', 'gene', 'strand', 'gene_start', 'gene_end']
    pd.testing.assert_frame_equal(out.drop(columns='strand'), plain)
    assert out.groupby('gene').strand.nunique().max() == 1 and set(out.strand) == {'+', '-'}
    # one exon line of the first gene says '.', every line of the second '?': both genes leave
    at = sc.exon_lines(data)
    first, second = out.gene.iloc[0], [g for g in out.gene.unique() if g != out.gene.iloc[0]][0]
    lines = data.split(b'\n')
    gene_lines = {g: [k for k in at if (g.encode() + b'"' in lines[k - 1]) or (b'=' + g.encode() + b';' in lines[k - 1] + b';')] for g in (first, second)}
    assert gene_lines[first] and gene_lines[second]
    text = sc.with_field7(data, gene_lines[first][0], b'.')
    for k in gene_lines[second]:
        text = sc.with_field7(text, k, b'?')
    p = str(tmp_path / ('u' + os.path.splitext(path)[1]))
    with open(p, 'wb') as f:
        f.write(text)
    proc = GeneAnnotationProcessor(p, verbose=False, strand=True)
    left = proc.run()
    assert proc.unstranded_genes == [first, second]
    pd.testing.assert_frame_equal(left.reset_index(drop=True), out[~out.gene.isin([first, second])].reset_index(drop=True))
