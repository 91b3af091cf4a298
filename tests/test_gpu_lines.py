"""
One family of newline layouts through the three text units that share the line table of csrc/dn_lines.hpp (LineTable,
line_span): dn_gtf_scan (loaders.scan_window), the GFF3 scan (loaders.gff3_scan, Gff3Scan.window) and dn_sam_encode
(bam.sam_records).  A break in the shared table must show in each of them.

The texts are at most three 16 KiB tiles long and made of valid lines of the unit's format, padded (attribute filler, a Z
tag for SAM) so that a '\\n' falls on bytes 63, 64, 65 (a lane's 64-byte share), 16383, 16384, 16385 (a tile edge), 32767 and
32768; with empty lines next to those bytes (GTF and GFF3: SAM rejects an empty line), with and without a final '\\n', and one
text of exactly 16384 bytes.  GFF3 texts also go through Gff3Scan.window in pieces cut at line ends, so that windows start
at offsets 1, 64 and 16383 of a tile (lines of the window before in the first tile: n_head > 0), and must give the rows of one
window.  The yardsticks are the plain-Python restatements (_gtf_fixtures.restate, _gff3_fixtures.restate, _sam_cases.encode),
computed once; test_texts_are_valid_for_their_restatements holds every generated text to them on the CPU first.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gff3_fixtures as g3                                            # noqa: E402
import _gtf_fixtures as gf                                             # noqa: E402
import _sam_cases as sc                                                # noqa: E402
from degnorm_amd import bam, loaders                                   # noqa: E402

TILE = 16384
# name -> (bytes that hold a '\n', in order; whether the text ends with the last of them).  Consecutive bytes: empty lines.
LAYOUTS = {'lane_63': ([63, 16383, 32767], True),
           'lane_64_open': ([64, 16384, 32768], False),
           'lane_65': ([65, 16385], True),
           'one_tile_exactly': ([16383], True),
           'one_tile_open': ([16383], False)}
EMPTY_LAYOUTS = {'empty_lines': ([63, 64, 65, 16383, 16384, 16385, 32767, 32768], True),
                 'empty_lines_open': ([63, 64, 65, 16383, 16384, 16385, 32767, 32768], False),
                 'window_starts': ([63, 16382, 16383, 16384, 32766], True)}       # pieces start at offsets 64, 16383 and 1 of a tile


def _gtf_line(k, pad):
    kind = ('exon', 'CDS', 'Exon')[k % 3]
    return 'c{0}\tt\t{1}\t{2}\t{3}\t.\t+\t.\tgene_id "I{4}"; gene_name "G{4}"; n '.format(k % 4, kind, k + 1, k + 9, k // 3).encode() + b'x' * pad


def _gff3_line(k, pad):
    j = k // 3                                                            # a gene, its transcript, an exon that names the transcript
    kind, attrs = (('gene', 'ID=g{0};Name=N{0}'), ('mRNA', 'ID=t{0};Parent=g{0}'), ('exon', 'Parent=t{0}'))[k % 3]
    return 'c{0}\tt\t{1}\t{2}\t{3}\t.\t+\t.\t{4};n='.format(j % 4, kind, k + 1, k + 9, attrs.format(j)).encode() + b'x' * pad


def _sam_line(k, pad):
    return sc.line(qname='q{0}'.format(k), rname=sc.REFS[k % 3][0], pos=1 + 7 * k, aux=('XZ:Z:' + 'z' * pad,))


def build(make, newlines, closed):
    """Lines of make(k, pad) with a '\\n' on every byte of `newlines`; not `closed`: one more line without its '\\n'."""
    widest = len(make(10 ** 4, 0))
    out, pos, k = [], 0, 0
    for t in newlines:
        gap = t - pos                                                    # bytes in front of the '\n' at t; none: an empty line
        while gap > 0:
            base = len(make(k, 0))
            if gap - (base + 1) >= widest:                               # a plain line with its '\n': room for the padded one stays
                out.append(make(k, 0) + b'\n')
                gap -= base + 1
            else:
                assert gap >= base
                out.append(make(k, gap - base))
                gap = 0
            k += 1
        out.append(b'\n')
        pos = t + 1
    text = b''.join(out) + (b'' if closed else make(k, 5))
    assert [p for p in newlines if text[p:p + 1] != b'\n'] == [] and len(text) <= 3 * TILE
    return text


def _texts(make, layouts):
    return {name: build(make, nl, closed) for name, (nl, closed) in layouts.items()}


GTF = _texts(_gtf_line, dict(LAYOUTS, **EMPTY_LAYOUTS))
GFF3 = _texts(_gff3_line, dict(LAYOUTS, **EMPTY_LAYOUTS))
SAM = _texts(_sam_line, LAYOUTS)
# the restatements, once
GTF_WANT = {name: gf.restate(text) for name, text in GTF.items()}
GFF3_WANT = {name: g3.restate(text) for name, text in GFF3.items()}
SAM_WANT = {name: sc.encode(text) for name, text in SAM.items()}


def test_texts_are_valid_for_their_restatements():
    assert len(GTF['one_tile_exactly']) == len(GFF3['one_tile_exactly']) == len(SAM['one_tile_exactly']) == TILE
    for texts, wants in ((GTF, GTF_WANT), (GFF3, GFF3_WANT)):
        for name, text in texts.items():
            nl, closed = dict(LAYOUTS, **EMPTY_LAYOUTS)[name]
            n_lines, no, chrs, starts, ends, genes = wants[name]
            assert text.endswith(b'\n') == closed and all(text[p] == 10 for p in nl)
            assert n_lines == text.count(b'\n') + (0 if closed else 1) and len(no) >= n_lines // 4 > 0
            assert (b'\n\n' in text) == (name in EMPTY_LAYOUTS)
    for name, text in SAM.items():
        stream, offs = SAM_WANT[name]
        assert len(offs) - 1 == text.count(b'\n') + (0 if LAYOUTS[name][1] else 1) and offs[-1] == len(stream) > 0


def _spans(data, beg, length):
    return [bytes(data[b:b + n]) for b, n in zip(beg.tolist(), length.tolist())]


def _assert_rows(data, cols, want):
    n_lines, no, chrs, starts, ends, genes = want
    assert cols['line'].tolist() == no and cols['start'].tolist() == starts and cols['end'].tolist() == ends
    assert _spans(data, cols['chr_beg'], cols['chr_len']) == chrs and _spans(data, cols['gene_beg'], cols['gene_len']) == genes


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(GTF))
def test_gtf_scan_equals_the_restatement(name):
    n_lines, cols, err, _, _ = loaders.scan_window(GTF[name], device=0)
    assert err is None and n_lines == GTF_WANT[name][0]
    _assert_rows(GTF[name], cols, GTF_WANT[name])


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(GFF3))
def test_gff3_scan_equals_the_restatement_in_one_window_and_in_pieces(name):
    data, want = GFF3[name], GFF3_WANT[name]
    n_lines, whole, err = loaders.gff3_scan(data, device=0)
    assert err is None and n_lines == want[0]
    _assert_rows(data, whole, want)
    cuts = [0] + [p + 1 for p in dict(LAYOUTS, **EMPTY_LAYOUTS)[name][0] if p + 1 < len(data)] + [len(data)]
    if name == 'window_starts':
        assert {1, 64, TILE - 1} <= {c % TILE for c in cuts}
    with loaders.Gff3Scan(len(data), 0) as scan:
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            cols, err, _, _ = scan.window(data[a:b])
            assert err is None
            parts.append(cols)
        cols = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        err, _, walked = loaders._resolve_pending(scan, cols)
        assert err is None and walked == int(cols['pending'].sum()) > 0 and scan.lines == want[0]
    for k in whole:
        assert np.array_equal(cols[k], whole[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SAM))
def test_sam_records_equal_the_restatement(name):
    stream, offs = bam.sam_records(SAM[name], sc.REFS, device=0)
    assert stream == SAM_WANT[name][0] and np.array_equal(offs, SAM_WANT[name][1])
