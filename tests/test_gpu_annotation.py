"""
GPU tests of the annotation stage (degnorm_amd.loaders / csrc/dn_gtf.hip, degnorm_amd.gene_processing) against the
reference's goldens (tests/golden/annotation.npz, made by tests/golden/make_golden_pipeline.py).

hard.gtf holds what a scanner gets wrong first: gene_name before and after gene_id, gene_id alone, an empty gene_name that
falls through to gene_id, `Exon` / `EXON`, CDS / transcript / gene lines, exact duplicate exon lines and duplicates that
differ only in the transcript, overlapping exons, a gene on two chromosomes, the names AB1 and AB10, chromosome names 1,
10, X and chrUn_gl000220, attributes without a trailing `;` and with blanks around `;`, a line of about 100 KB and a last
line without a newline.  The same files with `#` lines, blank lines and \\r\\n ends must give the same tables, malformed
lines must be named by number and kind, small windows and repeated runs must change nothing, and a file of 200 MB is
compared row for row with the plain Python restatement of tests/_gtf_fixtures.py.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gtf_fixtures as gf                                             # noqa: E402
from conftest import golden, GOLDEN                                    # noqa: E402
from test_annotation_host import DATA_COLS, FIXTURES, RUN_COLS, assert_same_table, golden_frame     # noqa: E402
from degnorm_amd import loaders                                        # noqa: E402
from degnorm_amd.gene_processing import GeneAnnotationProcessor        # noqa: E402
from degnorm_amd.loaders import GeneAnnotationLoader                   # noqa: E402

pytestmark = pytest.mark.gpu


def _path(name):
    return os.path.join(GOLDEN, name + '.gtf')


@pytest.mark.parametrize('name', FIXTURES)
def test_tables_equal_reference(name):
    z = golden('annotation')
    assert_same_table(GeneAnnotationLoader(_path(name)).get_data(), golden_frame(z, name + '_data', DATA_COLS))
    assert_same_table(GeneAnnotationProcessor(_path(name), verbose=False).run(), golden_frame(z, name + '_run', RUN_COLS))


def test_chromosome_subset_equals_reference():
    z = golden('annotation')
    got = GeneAnnotationProcessor(_path('hard'), chroms=['1', 'X'], verbose=False).run()
    assert_same_table(got, golden_frame(z, 'hard_sub_run', RUN_COLS))
    with pytest.raises(ValueError, match='Chromosome subsetting resulted in an empty DataFrame!'):
        GeneAnnotationProcessor(_path('hard'), chroms=['chr99'], verbose=False).run()


@pytest.mark.parametrize('name', FIXTURES)
@pytest.mark.parametrize('crlf', [False, True])
def test_header_lines_blank_lines_and_crlf_change_nothing(name, crlf, tmp_path):
    z = golden('annotation')
    noisy = str(tmp_path / 'noisy.gtf')
    gf.with_noise(_path(name), noisy, crlf=crlf)
    assert_same_table(GeneAnnotationLoader(noisy).get_data(), golden_frame(z, name + '_data', DATA_COLS))
    assert_same_table(GeneAnnotationProcessor(noisy, verbose=False).run(), golden_frame(z, name + '_run', RUN_COLS))


@pytest.mark.parametrize('name', FIXTURES)
def test_small_windows_and_repeated_runs_are_identical(name, monkeypatch):
    z = golden('annotation')
    expect = golden_frame(z, name + '_data', DATA_COLS)
    whole = GeneAnnotationLoader(_path(name))
    small = GeneAnnotationLoader(_path(name), window_bytes=4096)               # lines straddle the windows
    a, b, c = whole.get_data(), small.get_data(), small.get_data()
    for got in (a, b, c):
        assert_same_table(got, expect)
    codes = [ld.exon_codes() for ld in (small, small)]
    for x, y in zip(*codes):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    assert small.timing['bytes'] == os.path.getsize(_path(name)) and small.timing['lines'] == whole.timing['lines']
    monkeypatch.setattr(loaders, 'WINDOW_BYTES', 4096)
    assert_same_table(GeneAnnotationProcessor(_path(name), verbose=False).run(), golden_frame(z, name + '_run', RUN_COLS))


def _lines():
    with open(_path('pipeline'), 'rb') as f:
        return f.read().split(b'\n')[:-1]


EXON = b'chr1\ttest\texon\t101\t300\t.\t+\t.\t'
BAD = [('fields', b'chr1\ttest\tgene\t101\t300', 'must have the 9 mandatory .gtf columns'),
       ('fields', b'chr1\ttest\texon\t101\t300\t.\t+\t.', 'must have the 9 mandatory .gtf columns'),
       ('fields', b'just some text', 'must have the 9 mandatory .gtf columns'),
       ('gene', EXON + b'transcript_id "T1"; exon_number 1;', 'gene_name or gene_id'),
       ('gene', EXON + b'gene_name ""; gene_id " ";', 'gene_name or gene_id'),
       ('gene', EXON, 'gene_name or gene_id'),
       ('integer', b'chr1\ttest\texon\t10a\t300\t.\t+\t.\tgene_id "A";', 'not an integer'),
       ('integer', b'chr1\ttest\tEXON\t101\t\t.\t+\t.\tgene_id "A";', 'not an integer'),
       ('integer', b'chr1\ttest\texon\t1e3\t3000\t.\t+\t.\tgene_id "A";', 'not an integer'),
       ('integer', b'chr1\ttest\texon\t-5\t300\t.\t+\t.\tgene_id "A";', 'not an integer')]


@pytest.mark.parametrize('kind,bad,text', BAD, ids=['{0}{1}'.format(b[0], k) for k, b in enumerate(BAD)])
@pytest.mark.parametrize('window', [None, 256])
def test_malformed_lines_are_named(kind, bad, text, window, tmp_path):
    lines = _lines()
    for at in (0, 17, len(lines)):                                           # first line, in the middle, last line
        for tail in (b'\n', b''):
            p = str(tmp_path / 'bad.gtf')
            with open(p, 'wb') as f:
                f.write(b'\n'.join(lines[:at] + [bad] + lines[at:] + [bad]) + tail)      # the first one is the one reported
            with pytest.raises(ValueError) as e:
                GeneAnnotationLoader(p, window_bytes=window).get_data()
            msg = str(e.value)
            assert p in msg and 'line {0} '.format(at + 1) in msg and text in msg, msg
            with pytest.raises(ValueError, match='restated'):
                try:
                    gf.restate(open(p, 'rb').read())
                except ValueError as r:
                    assert r.args[0] == (at + 1, kind)
                    raise ValueError('restated')


def test_a_non_integer_outside_exon_lines_is_no_error(tmp_path):
    p = str(tmp_path / 'ok.gtf')
    with open(p, 'wb') as f:
        f.write(b'chr1\ttest\tgene\t.\tNA\t.\t+\t.\tnote "no gene tag";\n' + EXON + b'gene_id "A";\n')
    assert GeneAnnotationLoader(p).get_data().values.tolist() == [['chr1', 101, 300, 'A']]


EDGES = {'newlines only': (b'\n\n\n\n', 0), 'one comment, no newline': (b'#only a comment', 0), 'crlf blanks': (b'\r\n#x\r\n\r\n', 0),
         'one line, no newline': (EXON + b'gene_id "A"', 1), 'one line ending in cr': (EXON + b'gene_id "A"\r', 1),
         'one crlf line': (EXON + b'gene_id "A"\r\n', 1),
         'blank lines over several tiles': (b'\n' * 70000 + EXON + b'gene_name A;' + b'\n' * 70000, 1),
         'a 300 KB line': (EXON + b';' * 300000 + b'gene_name "far away"', 1)}


@pytest.mark.parametrize('case', sorted(EDGES))
def test_edges_of_the_buffer(case, tmp_path):
    data, rows = EDGES[case]
    p = str(tmp_path / 'edge.gtf')
    with open(p, 'wb') as f:
        f.write(data)
    for window in (None, 4096):
        ld = GeneAnnotationLoader(p, window_bytes=window)
        df = ld.get_data()
        n_lines, no, chrs, starts, ends, genes = gf.restate(data)
        assert len(df) == rows == len(no) and ld.timing['lines'] == n_lines
        assert df.gene.tolist() == [g.decode() for g in genes] and df.start.tolist() == starts


def test_two_hundred_megabytes_equal_the_restatement(tmp_path):
    p = str(tmp_path / 'big.gtf')
    n_lines, n_genes, size = gf.write_gtf(p, 11, 200 << 20)
    assert size >= 200 << 20
    ld = GeneAnnotationLoader(p, window_bytes=64 << 20)
    chr_code, start, end, gene_code, chr_names, gene_names = ld.exon_codes()
    assert ld.timing['lines'] == n_lines and ld.timing['bytes'] == size
    with open(p, 'rb') as f:
        r_lines, no, chrs, starts, ends, genes = gf.restate(f.read())
    assert r_lines == n_lines and len(no) == len(start) > 200000
    assert np.array_equal(start, np.array(starts)) and np.array_equal(end, np.array(ends))
    assert np.array(chr_names, dtype=object)[chr_code].tolist() == [c.decode() for c in chrs]
    assert np.array(gene_names, dtype=object)[gene_code].tolist() == [g.decode() for g in genes]
    assert len(gene_names) == len(set(genes)) == n_genes and len(chr_names) == len(gf.CHROMS)     # one string per distinct name
    # the frame on top of it: duplicates (exons shared by transcripts) dropped, the first one kept
    df = ld.get_data()
    want = pd.DataFrame({'chr': [c.decode() for c in chrs], 'start': starts, 'end': ends, 'gene': [g.decode() for g in genes]})
    assert_same_table(df, want.drop_duplicates().reset_index(drop=True))
    print('scan of {0} bytes: device {1:.1f} ms, copy-in {2:.1f} ms, file read {3:.2f} s'.format(
        size, ld.timing['device_ms'], ld.timing['copy_ms'], ld.timing['read_s']))
