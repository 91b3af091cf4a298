"""
The host build of the GFF3 scan (dn_gff3_scan_host through loaders.gff3_scan, no device) against the plain Python restatement
of the rule in tests/_gff3_fixtures.py: rows and errors alike, on the three dialects at size, on small texts that reach every
branch, and on 2 000 seeded mutations of a small file.  Also the dispatch by extension (loaders.annotation_loader).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gff3_fixtures as g3                                            # noqa: E402
from conftest import GOLDEN                                            # noqa: E402
from degnorm_amd import loaders                                        # noqa: E402


def scan_rows(data, device=None, hash_bits=64, stats=None):
    """gff3_scan in the shape of g3.restate: names as bytes cut out of data; an error as ValueError((line, kind name))."""
    n_lines, cols, err = loaders.gff3_scan(data, device=device, hash_bits=hash_bits, stats=stats)
    if err is not None:
        assert all(v.size == 0 for v in cols.values())
        raise ValueError((err[0], {v: k for k, v in g3.KINDS.items()}[err[1]]))
    chrs = [data[b:b + n] for b, n in zip(cols['chr_beg'].tolist(), cols['chr_len'].tolist())]
    genes = [data[b:b + n] for b, n in zip(cols['gene_beg'].tolist(), cols['gene_len'].tolist())]
    for name, h in zip(chrs + genes, cols['chr_hash'].tolist() + cols['gene_hash'].tolist()):
        assert h == fnv1a(name)
    return n_lines, cols['line'].tolist(), chrs, cols['start'].tolist(), cols['end'].tolist(), genes


_FNV = {}


def fnv1a(name):
    if name not in _FNV:
        h = 0xcbf29ce484222325
        for c in name:
            h = ((h ^ c) * 0x100000001b3) & 0xffffffffffffffff
        _FNV[name] = h
    return _FNV[name]


@pytest.mark.parametrize('dialect', g3.DIALECTS)
def test_dialects_at_size_equal_the_restatement(dialect, tmp_path):
    _, path = g3.write_twin(str(tmp_path), 3, 400000, dialect)         # the .gtf is the larger twin: about 200 KB of GFF3
    data = open(path, 'rb').read()
    assert len(data) > 150000
    stats = {}
    got, want = g3.outcome(scan_rows, data, stats=stats), g3.outcome(g3.restate, data)
    assert want[0] == 'rows' and len(want[2]) > 300 and got == want
    assert stats['nodes'] > 300
    if dialect == 'ensembl':
        assert stats['walked_exons'] == len(want[2])                   # every exon names only its transcript
    else:
        assert 0 < stats['walked_exons'] < len(want[2]) // 2           # the exons of the genes without a name
    assert g3.outcome(scan_rows, data, hash_bits=4) == want
    # and as a noisy copy: blank lines, CRLF
    noisy = b'\r\n'.join(sum(([ln, b''] if k % 7 == 0 else [ln] for k, ln in enumerate(data.split(b'\n')[:-1])), [])) + b'\r\n'
    assert g3.outcome(scan_rows, noisy) == g3.outcome(g3.restate, noisy)


@pytest.mark.parametrize('name', sorted(g3.CASES))
def test_small_texts_equal_the_restatement(name):
    data = g3.CASES[name]
    want = g3.outcome(g3.restate, data)
    assert want[0] == 'rows', name
    for bits in (64, 4, 1):
        assert g3.outcome(scan_rows, data, hash_bits=bits) == want, (name, bits)


def test_what_the_small_texts_are_meant_to_show():
    rows = {name: g3.outcome(g3.restate, data)[2] for name, data in g3.CASES.items()}
    genes = {name: [r[4] for r in v] for name, v in rows.items()}
    assert genes['ensembl_small'] == [b'ALPHA', b'ALPHA'] and genes['children_first'] == [b'ALPHA', b'ALPHA']
    assert genes['fasta_tail'] == [b'ALPHA'] and rows['fasta_crlf_first'] == [] and genes['not_quite_fasta'] == [b'OWN']
    assert genes['several_parents'] == [b'BETA', b'ALPHA', b'FALLBACK']
    assert genes['repeated_ids'] == [b'FIRST']
    assert genes['spaces'] == [b'SPACED NAME', b'A=B']
    assert genes['empty_values'] == [b'GID', b'g2', b'THIRD', b'X']
    assert genes['gene_against_gene_id'] == [b'YES', b'ID2', b'RN']
    assert genes['chain_8'] == [b'TOP'] and genes['gname_midway'] == [b'MID'] and genes['tenth_field'] == [b'N']
    assert genes['headers_blank_crlf'] == [b'ALPHA', b'OWN'] and [r[0] for r in rows['headers_blank_crlf']] == [8, 10]
    assert rows['big_integers'] == [(1, b'c1', 7, 10 ** 18 - 1, b'G')]
    assert len(rows['many_lines']) == 520


@pytest.mark.parametrize('name', sorted(g3.ERRORS))
def test_errors_have_their_line_and_kind(name):
    data, line, kind = g3.ERRORS[name]
    assert g3.outcome(g3.restate, data) == ('error', line, kind), name
    for bits in (64, 4):
        assert g3.outcome(scan_rows, data, hash_bits=bits) == ('error', line, kind), (name, bits)
    assert loaders._GFF3_KINDS[g3.KINDS[kind]] == g3.TEXT[kind]


def test_hash_bits_fill_the_runs_and_change_nothing():
    data = g3.CASES['many_lines']
    want = g3.outcome(scan_rows, data)
    for bits in (1, 2, 4, 8, 63):
        assert g3.outcome(scan_rows, data, hash_bits=bits) == want
    with pytest.raises(ValueError):
        loaders.gff3_scan(data, hash_bits=0)
    with pytest.raises(ValueError):
        loaders.gff3_scan(data, hash_bits=65)
    assert loaders.gff3_scan(b'')[0] == 0


def test_mutations_give_rows_or_a_status_equal_to_the_restatement():
    n = {'rows': 0, 'error': 0}
    for data in g3.mutations(2000):
        want = g3.outcome(g3.restate, data)
        assert g3.outcome(scan_rows, data) == want, data
        n[want[0]] += 1
    assert n['rows'] > 200 and n['error'] > 200


def test_annotation_loader_picks_the_class_by_extension(tmp_path):
    from degnorm_amd.gene_processing import GeneAnnotationProcessor
    for ext, cls in (('.gtf', loaders.GeneAnnotationLoader), ('.gff3', loaders.Gff3AnnotationLoader), ('.gff', loaders.Gff3AnnotationLoader)):
        p = tmp_path / ('genes' + ext)
        p.write_bytes(g3.CASES['ensembl_small'])
        got = loaders.annotation_loader(str(p), window_bytes=4096)
        assert type(got) is cls and got.filename == str(p) and got.window_bytes == 4096
    other = tmp_path / 'genes.bed'
    other.write_text('x\n')
    with pytest.raises(ValueError, match='does not end with .gtf, .gff3, .gff'):
        loaders.annotation_loader(str(other))
    with pytest.raises(FileNotFoundError, match='not found'):
        loaders.annotation_loader(str(tmp_path / 'missing.gff3'))
    with pytest.raises(ValueError, match='data type not understood'):
        loaders.annotation_loader(17)
    # the GTF loader keeps to its own format
    with pytest.raises(ValueError, match='does not end with .gtf'):
        loaders.GeneAnnotationLoader(str(tmp_path / 'genes.gff3'))
    with pytest.raises(ValueError, match='does not end with .gff3, .gff'):
        loaders.Gff3AnnotationLoader(os.path.join(GOLDEN, 'chr1_small.gtf'))
    gap = GeneAnnotationProcessor(str(tmp_path / 'genes.gff3'), verbose=False)
    assert gap.loader is None and gap.filename.endswith('.gff3')


def test_file_loader_has_no_cpu_fallback(tmp_path):
    from degnorm_amd import _lib
    p = tmp_path / 'genes.gff3'
    p.write_bytes(g3.CASES['ensembl_small'])
    if _lib.device_count() > 0:                                        # a GPU is visible here: the loader loads
        assert loaders.Gff3AnnotationLoader(str(p)).get_data().gene.tolist() == ['ALPHA', 'ALPHA']
        return
    with pytest.raises(_lib.DegnormAmdError):
        loaders.Gff3AnnotationLoader(str(p)).get_data()


def test_pipeline_fixture_names_the_genes_of_the_gtf_fixture(tmp_path):
    import _gtf_fixtures as gf
    gf.write_pipeline_gtf(str(tmp_path / 'p.gtf'))
    g3.write_pipeline_gff3(str(tmp_path / 'p.gff3'))
    a = gf.restate(open(str(tmp_path / 'p.gtf'), 'rb').read())
    data = open(str(tmp_path / 'p.gff3'), 'rb').read()
    b = g3.restate(data)
    assert list(zip(*a[2:])) == list(zip(*b[2:]))
    assert g3.outcome(scan_rows, data) == g3.outcome(g3.restate, data)
