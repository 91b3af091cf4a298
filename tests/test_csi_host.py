"""
Host tests of the .csi index (degnorm_amd.bam.build_index(fmt='csi') with device=None: the host build of csrc/dn_bai.hip; no
GPU): the inflated bytes against the pure-Python builder of tests/_csi_cases.py on every case, block layout and window
size; bins, chunks and offsets against the .bai of the same file at (14, 5); region queries against brute force over the
reads; parse_csi / read_index on the library's files and on hand-written variants; the errors; the command's arguments.
"""
import argparse
import gzip
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bai_cases as bc                                        # noqa: E402
import _bam_fixtures as bf                                     # noqa: E402
import _csi_cases as cc                                        # noqa: E402
from degnorm_amd import __main__ as cli                        # noqa: E402
from degnorm_amd import bam, utils                             # noqa: E402

PARAMS = cc.SHARED + [(name, cc.CASES[name][0], cc.CASES[name][1]) for name in sorted(cc.CASES)]


@pytest.fixture(scope='module')
def built(tmp_path_factory):
    """{(case, layout): (path, refs, records, blocks, reads)}, each written once."""
    d = tmp_path_factory.mktemp('csi')
    out = {}
    for name in sorted(bc.CASES) + sorted(cc.CASES):
        for layout in bc.LAYOUTS:
            p = str(d / '{0}_{1}.bam'.format(name, layout))
            out[name, layout] = (p,) + cc.build_case(name, layout, p, level=6 if layout == 'empty' else 1)
    return out


def _depth(refs, min_shift, depth):
    return cc.auto_depth(refs, min_shift) if depth is None else depth


def test_cases_cover_what_they_claim(built):
    tables = {name: bc.record_table(built[name, 'aligned'][2]) for name in cc.CASES}
    # levels: every level of (4, 3) holds a record, one record ends at the cap, every boundary of every level is straddled by one base
    got = set(cc.bin_level(cc.reg2bin(beg, end, 4, 3), 4, 3)[0] for ref, beg, end, flag, s, e in tables['levels'] if ref == 0)
    assert got == {0, 1, 2, 3}
    assert max(end for ref, beg, end, flag, s, e in tables['levels']) == 1 << 13 == built['levels', 'aligned'][1][0][1]
    spans = set((beg, end) for ref, beg, end, flag, s, e in tables['levels'] if ref == 0)
    for s in (4, 7, 10):
        assert any(end - beg == 2 and (beg + 1) % (1 << s) == 0 and ((beg + 1) >> s) % 8 for beg, end in spans), s
    assert min(end - beg for beg, end in spans) == 1 and max(end - beg for beg, end in spans) == 8191
    # wide: granules beyond 16 bits, in one record and between records; the spliced read from granule 10 to 131 100
    assert max((end - 1) >> 4 for ref, beg, end, flag, s, e in tables['wide']) > 65535
    assert any(beg >> 4 == 10 and (end - 1) >> 4 == 131100 for ref, beg, end, flag, s, e in tables['wide'] if ref == 0)
    assert any((end - 1) >> 4 == 65535 for ref, beg, end, flag, s, e in tables['wide'])
    assert any(beg >> 4 == 65536 for ref, beg, end, flag, s, e in tables['wide'])
    assert sum(beg >> 4 > 65536 and end - beg < 100 for ref, beg, end, flag, s, e in tables['wide'] if ref == 1) > 300
    # beyond: past the .bai's cap, around it on both sides, up to the last base; depth=None is 6
    refs = built['beyond', 'aligned'][1]
    H = 1 << 29
    assert max(end for ref, beg, end, flag, s, e in tables['beyond']) == refs[0][1] > H
    have = set((beg, end) for ref, beg, end, flag, s, e in tables['beyond'] if ref == 0)
    assert (H - 50, H) in have and (H - 1, H + 1) in have and (H, H + 50) in have and (H - 20000, H + 20050) in have
    assert sum(beg < 1 << 20 for beg, end in have) >= 290 and cc.auto_depth(refs) == 6
    for name in cc.CASES:
        assert 2000 < len(tables[name]) < 5000 and len(built[name, 'aligned'][3]) > 8
    assert cc.auto_depth(built['three', 'aligned'][1]) == 2 and cc.auto_depth(built['deep', 'aligned'][1]) == 6


@pytest.mark.parametrize('layout', bc.LAYOUTS)
@pytest.mark.parametrize('name,min_shift,depth', PARAMS)
def test_host_build_equals_specification(built, name, min_shift, depth, layout):
    p, refs, records, blocks, reads = built[name, layout]
    spec = cc.spec_index(refs, records, blocks, min_shift, _depth(refs, min_shift, depth))
    for window_bytes in bc.WINDOWS:
        stats = {}
        idx = bam.build_index(p, window_bytes=window_bytes, n_jobs=2 if window_bytes else 1, stats=stats, fmt='csi', min_shift=min_shift,
                              depth=depth)
        assert idx.tobytes() == spec, (name, layout, window_bytes)
        assert (idx.fmt, idx.min_shift, idx.depth) == ('csi', min_shift, _depth(refs, min_shift, depth))
        assert stats['records'] == len(reads) and stats['chunks'] > 0
    assert idx.n_no_coor == int((reads.ref < 0).sum())


@pytest.mark.parametrize('name', sorted(bc.CASES))
def test_equals_the_bai_at_14_5(built, name):
    p = built[name, 'straddle'][0]
    csi, bai = bam.build_index(p, fmt='csi', depth=5), bam.build_index(p, fmt='bai')
    assert bai.fmt == 'bai' and bai.tobytes()[:4] == b'BAI\x01' and csi.pseudo_bin == bam.PSEUDO_BIN == 37450
    n = 0
    for tid in range(len(csi.refs)):
        a, b = csi.refs[tid], bai.refs[tid]
        assert [x[0] for x in a['bins']] == [x[0] for x in b['bins']] and csi.pseudo(tid) == bai.pseudo(tid)
        assert all(np.array_equal(x[1], y[1]) for x, y in zip(a['bins'], b['bins'])) and len(a['loffset']) == len(a['bins'])
        for (bin_id, _), loffset in zip(a['bins'], a['loffset']):
            if bin_id == 37450:
                assert loffset == 0
                continue
            start = cc.bin_level(bin_id, 14, 5)[1]
            assert loffset == int(b['ioffset'][start >> 14]), (tid, bin_id)
            n += 1
    assert n > 30


@pytest.mark.parametrize('name,min_shift,depth', PARAMS)
def test_region_queries(built, name, min_shift, depth):
    p, refs, records, blocks, reads = built[name, 'straddle']
    idx = bam.build_index(p, fmt='csi', min_shift=min_shift, depth=depth)
    table = [(ref, beg, end, bc.voffset(blocks, s)) for ref, beg, end, flag, s, e in bc.record_table(records)]
    if name in bc.CASES:
        regions = bc.regions(refs, reads, 200, seed=11)
    else:
        regions = cc.regions(name, refs, reads, 200, 12, idx.min_shift, idx.depth)
    n_hits = 0
    for tid, beg, end in regions:
        chunks = bam.index_chunks(idx, tid, beg, end)
        assert all(a < b for a, b in chunks) and all(x[1] < y[0] for x, y in zip(chunks[:-1], chunks[1:]))
        for ref, rb, re_, vb in table:
            if ref == tid and rb < end and re_ > beg:
                n_hits += 1
                assert any(a <= vb < b for a, b in chunks), (tid, beg, end, rb, re_)
    assert n_hits > 1000
    assert bam.reg2bins(5, 70000) == bc.reg2bins(5, 70000) and bam.reg2bins(0, 1 << 29) == bc.reg2bins(0, 1 << 29)


# --- the parser ------------------------------------------------------------------------------------------------------------

def _decode(b):
    min_shift, depth, l_aux = struct.unpack_from('<iii', b, 4)
    aux, p = b[16:16 + l_aux], 16 + l_aux
    n_ref = struct.unpack_from('<i', b, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from('<i', b, p)[0]
        p += 4
        bins = []
        for _ in range(n_bin):
            bin_id, loffset, n_chunk = struct.unpack_from('<IQi', b, p)
            bins.append((bin_id, loffset, b[p + 16:p + 16 + 16 * n_chunk]))
            p += 16 + 16 * n_chunk
        refs.append(bins)
    return min_shift, depth, aux, refs, b[p:]


def _encode(min_shift, depth, aux, refs, tail):
    out = b'CSI\x01' + struct.pack('<iii', min_shift, depth, len(aux)) + aux + struct.pack('<i', len(refs))
    for bins in refs:
        out += struct.pack('<i', len(bins))
        for bin_id, loffset, ch in bins:
            out += struct.pack('<IQi', bin_id, loffset, len(ch) // 16) + ch
    return out + tail


def _bgzf(path, data, block=0xff00, eof=True):
    with open(path, 'wb') as f:
        for k in range(0, len(data), block):
            f.write(bf._bgzf_block(data[k:k + block], 6))
        if eof:
            f.write(bf.EOF_BLOCK)
    return path


def test_parser_and_reader(built, tmp_path):
    import shutil
    src, refs, records, blocks, reads = built['three', 'aligned']
    p = str(tmp_path / 's.bam')
    shutil.copy(src, p)
    # the library's own files
    spec = cc.spec_index(refs, records, blocks, 14, 2)
    assert bam.create_index(p, fmt='csi') == p + '.csi'
    assert bam.has_eof_block(p + '.csi') and open(p + '.csi', 'rb').read(2) == b'\x1f\x8b'
    assert gzip.open(p + '.csi').read() == spec and bam.parse_csi(p + '.csi').tobytes() == spec
    with pytest.raises(FileExistsError):
        bam.create_index(p, fmt='csi')
    assert utils.create_index_file(p, fmt='csi', min_shift=4, depth=6) == str(tmp_path / 's.csi')
    small = bam.parse_csi(str(tmp_path / 's.csi'))
    assert (small.min_shift, small.depth) == (4, 6) and small.tobytes() == cc.spec_index(refs, records, blocks, 4, 6)
    assert len(small.tobytes()) > 0xff00 and len(bam.bgzf_blocks(str(tmp_path / 's.csi'))[0]) == 3      # two blocks and the end-of-file block
    plain, n_no_coor = bam.read_index(p + '.csi')
    assert n_no_coor == 150 and [bam.reference_range(r) is None for r in plain] == [False, True, False]
    theirs = bam.build_index(p)
    assert [r['pseudo'] for r in plain] == [theirs.pseudo(t) for t in range(3)]
    assert [bam.reference_range(r) for r in bam.read_index(str(tmp_path / 's.csi'))[0]] == [bam.reference_range(r) for r in plain]
    # a .bai goes to read_bai, messages and all
    bai = bam.create_index(p)
    assert bam.read_index(bai) == bam.read_bai(bai)
    with pytest.raises(ValueError, match='is not a .bai index'):
        bam.read_index(__file__)
    with pytest.raises(ValueError, match='is not a .csi index'):
        bam.parse_csi(bai)
    # hand-written variants of the same index
    min_shift, depth, aux, bins, tail = _decode(spec)
    assert _encode(min_shift, depth, aux, bins, tail) == spec and len(tail) == 8
    variants = {
        'aux': _encode(min_shift, depth, b'twelve bytes', bins, tail),
        'descending': _encode(min_shift, depth, aux, [b[::-1] for b in bins], tail),
        'no_tail': _encode(min_shift, depth, aux, bins, b''),
        'no_pseudo': _encode(min_shift, depth, aux, [b[:-1] for b in bins], tail),
        'blocks': spec,
    }
    for name, data in variants.items():
        path = _bgzf(str(tmp_path / (name + '.csi')), data, block=200 if name == 'blocks' else 0xff00)
        idx = bam.parse_csi(path)
        assert idx.tobytes() == data, name
        got, n = bam.read_index(path)
        assert [bam.reference_range(r) for r in got] == [bam.reference_range(r) for r in plain], name
        assert n == (None if name == 'no_tail' else 150)
        assert all(r['pseudo'] is None for r in got) if name == 'no_pseudo' else [r['pseudo'] for r in got] == [r['pseudo'] for r in plain]
    assert bam.parse_csi(str(tmp_path / 'aux.csi')).aux == b'twelve bytes' and len(bam.bgzf_blocks(str(tmp_path / 'blocks.csi'))[0]) > 5
    assert bam.parse_csi(str(tmp_path / 'descending.csi')).refs[0]['bins'][0][0] == cc.pseudo_bin(2)
    # the reader takes it
    proc = bam.NativeBamReadsProcessor(p, p + '.csi', verbose=False)
    assert proc.chroms == ['chrA', 'chrE', 'chrB']
    # files that are refused, by name
    raw = open(p + '.csi', 'rb').read()
    bad = {'cut.csi': raw[:-10], 'cut_mid.csi': raw[:len(raw) // 2]}
    for name, data in bad.items():
        open(str(tmp_path / name), 'wb').write(data)
    _bgzf(str(tmp_path / 'short.csi'), spec[:len(spec) // 2])
    _bgzf(str(tmp_path / 'short_head.csi'), spec[:14])
    for name in ('cut.csi', 'cut_mid.csi', 'short.csi', 'short_head.csi'):
        for fn in (bam.read_index, bam.parse_csi):
            with pytest.raises(ValueError) as e:
                fn(str(tmp_path / name))
            assert str(tmp_path / name) in str(e.value) and 'truncated .csi index' in str(e.value), (name, str(e.value))
    other = str(tmp_path / 'other.csi')
    open(other, 'wb').write(gzip.compress(b'something else entirely'))
    for fn in (bam.read_index, bam.parse_csi):
        with pytest.raises(ValueError, match='other.csi is not a .csi index'):
            fn(other)
    one = str(tmp_path / 'one.bam')
    bf.write_bam(one, [('chrA', 300000)], reads[reads.ref == 0], index=False)
    with pytest.raises(ValueError) as e:
        bam.NativeBamReadsProcessor(one, p + '.csi', verbose=False)
    assert str(e.value) == '{0} indexes 3 references, {1} has 1'.format(p + '.csi', one)


# --- errors ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('min_shift,depth', cc.RANGE_PARAMS)
def test_range_error(min_shift, depth, tmp_path):
    for extra in (0, 1):
        p = str(tmp_path / 'r{0}.bam'.format(extra))
        pos, text = cc.range_file(p, min_shift, depth, extra)
        for kw in bc.ERROR_SIZES:
            if extra == 0:                                            # an end exactly at the cap is held
                idx = bam.build_index(p, fmt='csi', min_shift=min_shift, depth=depth, **kw)
                assert idx.pseudo(0)[2] == 701
                continue
            with pytest.raises(ValueError) as e:
                bam.build_index(p, fmt='csi', min_shift=min_shift, depth=depth, **kw)
            assert str(e.value) == text


def test_errors(tmp_path):
    nowhere = str(tmp_path / 'no_such.bam')
    for kw in (dict(min_shift=0), dict(min_shift=31), dict(depth=-1), dict(depth=9), dict(min_shift=-3, depth=2)):
        for fn in (bam.build_index, bam.create_index):
            with pytest.raises(ValueError, match='min_shift|depth'):
                fn(nowhere, fmt='csi', **kw)
    with pytest.raises(ValueError, match="fmt must be 'bai' or 'csi'"):
        bam.build_index(nowhere, fmt='tbi')
    with pytest.raises(ValueError, match='a .bai index has min_shift 14 and depth 5'):
        bam.build_index(nowhere, min_shift=12)
    with pytest.raises(FileNotFoundError):
        bam.build_index(nowhere, fmt='csi')
    # the .bai texts have not moved, and the same files have the same faults as a .csi
    for name, (path, text) in bc.error_files(tmp_path).items():
        with pytest.raises(ValueError) as e:
            bam.build_index(path, fmt='bai')
        assert text in str(e.value) and str(e.value).startswith(path + ': '), (name, str(e.value))
        if name != 'beyond':
            with pytest.raises(ValueError) as e:
                bam.build_index(path, fmt='csi', depth=5)
            assert text in str(e.value), (name, str(e.value))
    path = bc.error_files(tmp_path)['beyond'][0]
    with pytest.raises(ValueError, match='reaches beyond position 2\\^29: a .csi index of min_shift 14 and depth 5 cannot hold it'):
        bam.build_index(path, fmt='csi', depth=5)
    assert bam.build_index(path, fmt='csi').depth == 6                # chrB has 2^29 bases: with 256 more, depth 6
    # no linear index to fetch offsets from, and no per-bin offsets in a .bai builder
    lib = bam._lib.load()
    import ctypes
    h = ctypes.c_void_p()
    assert lib.dn_bai_create(-1, 1, 0, ctypes.byref(h)) == 0
    sizes = np.zeros(8, np.int64)
    assert lib.dn_bai_finish(h, 0, sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
    assert lib.dn_csi_loffset(h, np.zeros(1, np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) != 0
    lib.dn_bai_destroy(h)
    for bad in ((0, 5), (31, 0), (14, 9), (14, -1)):
        assert lib.dn_csi_create(-1, 1, 0, bad[0], bad[1], ctypes.byref(h)) != 0


# --- the command ---------------------------------------------------------------------------------------------------------

def _args(**kw):
    base = dict(bam_files=None, bai_files=None, bam_dir=None, warm_start_dir=None, genome_annotation=None, output_dir=None,
                downsample_rate=1, nmf_iter=100, iter=5, minimax_coverage=0, skip_baseline_selection=False,
                non_unique_alignments=False, proc_per_node=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_command_line(tmp_path):
    d = str(tmp_path)
    gtf = os.path.join(d, 'a.gtf')
    open(gtf, 'w').close()
    bams = [os.path.join(d, 's{0}.bam'.format(k)) for k in (1, 2, 3)]
    for b in bams:
        open(b, 'w').close()
    ap = cli.argparser()
    ns = ap.parse_args(['--bam-dir', d, '-g', gtf, '--create-bai', '--index-format', 'csi'])
    assert ns.index_format == 'csi' and ap.parse_args(['--bam-dir', d, '-g', gtf]).index_format == 'bai'
    with pytest.raises(SystemExit):
        ap.parse_args(['--bam-dir', d, '-g', gtf, '--index-format', 'tbi'])
    ok = cli.validate_args(ns)
    assert ok.bai_files == [b[:-3] + 'csi' for b in bams] and ok.create_bai_files == bams and ok.index_format == 'csi'
    ok = cli.validate_args(ap.parse_args(['--bam-dir', d, '-g', gtf, '--create-bai']))
    assert ok.bai_files == [b[:-3] + 'bai' for b in bams] and ok.create_bai_files == bams and ok.index_format == 'bai'
    # the missing-index error keeps its text, with either format
    for extra in ([], ['--index-format', 'csi']):
        with pytest.raises(FileNotFoundError, match='No .bai index file .*s1.bai for .*s1.bam: pass --create-bai'):
            cli.validate_args(ap.parse_args(['--bam-dir', d, '-g', gtf] + extra))
    # discovery: X.bai before X.csi before X.bam.csi
    open(bams[0] + '.csi', 'w').close()
    open(bams[1] + '.csi', 'w').close()
    open(bams[1][:-3] + 'csi', 'w').close()
    for name in (bams[2] + '.csi', bams[2][:-3] + 'csi', bams[2][:-3] + 'bai'):
        open(name, 'w').close()
    want = [bams[0] + '.csi', bams[1][:-3] + 'csi', bams[2][:-3] + 'bai']
    for src in (dict(bam_files=bams), dict(bam_dir=d)):
        for kw in ({}, dict(create_bai=True, index_format='csi')):
            ok = cli.validate_args(_args(genome_annotation=gtf, **src, **kw))
            assert ok.bai_files == want and ok.create_bai_files == []
    # --bai-files takes .csi names
    ok = cli.validate_args(_args(bam_files=bams[:2], bai_files=[bams[0] + '.csi', bams[1][:-3] + 'csi'], genome_annotation=gtf))
    assert ok.bai_files == [bams[0] + '.csi', bams[1][:-3] + 'csi']
    txt = os.path.join(d, 'x.txt')
    open(txt, 'w').close()
    with pytest.raises(ValueError, match='x.txt is not a .bai file'):
        cli.validate_args(_args(bam_files=bams[:2], bai_files=[bams[0] + '.csi', txt], genome_annotation=gtf))
    assert '--index-format' in ap.format_help() and utils.index_from_bam_file('a/b.bam', 'csi') == 'a/b.csi'
