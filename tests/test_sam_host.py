"""
Host build of the SAM encoder (degnorm_amd.bam.sam_records / sam_to_bam with device=None; csrc/dn_sam.hip, dn_sam.hpp), no
device: every case of tests/_sam_cases.py against the plain-Python restatement of the definition in include/degnorm_amd.h,
byte for byte; every error with its line number and text; the written files (header, blocks, end-of-file block, nothing left
behind on an error); and the fixture rows of _bam_fixtures converted, sorted and indexed on the host and read back.
"""
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _sam_cases as sc                                        # noqa: E402
from degnorm_amd import bam, utils                             # noqa: E402


def inflate_file(path):
    return b''.join(bam.inflate_block(b) for _, b in bam.iter_blocks(path))


def test_the_cases_are_what_they_claim():
    assert len(sc.lines_of(sc.VALID['n255'])) == 255 and len(sc.lines_of(sc.VALID['n257'])) == 257
    text, pos, straddles = sc.VALID['straddle_tile'], 0, False
    for ln in text.split(b'\n')[:-1]:
        straddles |= pos < sc.TILE < pos + len(ln)
        pos += len(ln) + 1
    assert straddles
    assert max(len(ln) for ln in sc.lines_of(sc.VALID['long_line'])) > sc.TILE
    # the float whose nearest double and nearest float differ: above the midpoint of 1 and 1 + 2^-23, nearer to the midpoint than
    # to any other double
    fl = sc.double_rounding_text()
    mid = 1 + Fraction(1, 2 ** 24)
    assert mid < Fraction(fl) < mid + Fraction(1, 2 ** 54) and float(fl) == float(mid)
    assert struct.pack('<f', float(fl)) == struct.pack('<f', 1.0)
    stream, _ = sc.encode(sc.line(aux=('Xr:f:' + fl,)))
    assert stream.endswith(b'Xrf' + struct.pack('<f', 1.0))
    # every DN_SAM_E_* of the header has the text the tests expect, and the other way round
    assert sorted(bam.SAM_ERRORS.values()) == sorted(sc.TEXT.values())


@pytest.mark.parametrize('name', sorted(sc.VALID))
def test_records_equal_the_restatement(name):
    text = sc.VALID[name]
    expect, expect_off = sc.encode(text)
    stats = {}
    stream, off = bam.sam_records(text, sc.REFS, stats=stats)
    assert stream == expect and off.tolist() == expect_off.tolist()
    assert stats['lines'] == stats['records'] == len(expect_off) - 1 and stats['encode_device_ms'] == 0.0
    if name in sc.N_LINES:
        assert stats['records'] == sc.N_LINES[name]
    # what the reader's framing makes of the stream: the same records
    got, used, _ = bam.frame_records(stream)
    assert got.tolist() == expect_off[:-1].tolist() and used == len(stream)


def test_float_patches_are_counted():
    stats = {}
    bam.sam_records(sc.VALID['tag_f'], sc.REFS, stats=stats)
    assert stats['float_patches'] == 11 + 3 + 1                 # eleven f fields and a B:f of three, and one f on the last line
    bam.sam_records(sc.VALID['one'], [n for n, _ in sc.REFS], stats=stats)
    assert stats['float_patches'] == 0


@pytest.mark.parametrize('name', sorted(sc.ERRORS))
def test_errors_name_the_line(name):
    text, line, kind = sc.ERRORS[name]
    with pytest.raises(sc.SamFault) as spec:
        sc.encode(text)
    assert (spec.value.line, spec.value.kind) == (line, kind)
    with pytest.raises(ValueError) as e:
        bam.sam_records(text, sc.REFS)
    assert str(e.value) == 'line {0}: {1}'.format(line, sc.TEXT[kind])


@pytest.mark.parametrize('deflate', ['zlib', 'native'])
@pytest.mark.parametrize('window_bytes', [None, 1, 4096])
def test_files_equal_the_restatement(tmp_path, window_bytes, deflate):
    kw = {} if window_bytes is None else {'window_bytes': window_bytes}
    for name in sorted(sc.VALID):
        if window_bytes == 1 and name in ('n255', 'n256', 'straddle_tile'):
            continue                                            # one window per line: n257 has the many-window case
        text = sc.VALID[name]
        src, dst = sc.write_sam(str(tmp_path / (name + '.sam')), text), str(tmp_path / (name + '.bam'))
        stats = {}
        assert bam.sam_to_bam(src, dst, deflate=deflate, stats=stats, **kw) == dst
        stream, off = sc.encode(text)
        assert inflate_file(dst) == sc.bam_header(sc.HEADER, sc.REFS) + stream, name
        assert bam.has_eof_block(dst) and not os.path.exists(dst + '.tmp')
        assert bam.verify_bgzf(dst)['inflated_bytes'] == len(sc.bam_header(sc.HEADER, sc.REFS)) + len(stream)
        assert bam.read_header(dst) == sc.REFS
        data = bam._header_data(dst)[0]
        assert data[8:8 + struct.unpack_from('<i', data, 4)[0]] == sc.HEADER.encode()
        n = len(off) - 1
        assert stats['lines'] == stats['records'] == n and stats['record_bytes'] == len(stream) and stats['encode_device_ms'] == 0.0
        assert stats['bytes_in'] == os.path.getsize(src) and stats['bytes_out'] == os.path.getsize(dst)
        assert (stats['windows'] >= 1) == (n > 0) and (window_bytes != 1 or stats['windows'] == n)
        # no block holds more than 0xff00 bytes, and a block ends where a record ends unless the record is longer than a block
        ends, at = set(off.tolist()), len(sc.bam_header(sc.HEADER, sc.REFS))
        for isize in bam.bgzf_blocks(dst)[2].tolist()[1:-1]:
            at += isize
            assert isize <= 0xff00 and (at - len(sc.bam_header(sc.HEADER, sc.REFS)) in ends or isize == 0xff00)


def test_threads_and_overwrite(tmp_path):
    src = sc.write_sam(str(tmp_path / 'a.sam'), sc.VALID['cigar_65535'] + sc.VALID['n257'])
    one, four = str(tmp_path / 'one.bam'), str(tmp_path / 'four.bam')
    bam.sam_to_bam(src, one)
    bam.sam_to_bam(src, four, n_jobs=4)
    assert open(one, 'rb').read() == open(four, 'rb').read()
    with pytest.raises(FileExistsError):
        bam.sam_to_bam(src, one)
    assert bam.sam_to_bam(src, one, overwrite=True) == one
    with pytest.raises(ValueError, match='deflate must be'):
        bam.sam_to_bam(src, one, deflate='gzip', overwrite=True)
    assert utils.sam_to_bam_file(src) == str(tmp_path / 'a.bam') and open(str(tmp_path / 'a.bam'), 'rb').read() == open(one, 'rb').read()
    with pytest.raises(ValueError, match='must have a .sam extension'):
        utils.sam_to_bam_file(one)


@pytest.mark.parametrize('window_bytes', [None, 1, 4096])
def test_file_errors_name_file_and_line_and_leave_nothing(tmp_path, window_bytes):
    kw = {} if window_bytes is None else {'window_bytes': window_bytes}
    n_head = sc.HEADER.count('\n')
    for name, (text, line, kind) in sorted(sc.ERRORS.items()):
        src, dst = sc.write_sam(str(tmp_path / (name + '.sam')), text), str(tmp_path / (name + '.bam'))
        with pytest.raises(ValueError) as e:
            bam.sam_to_bam(src, dst, **kw)
        assert str(e.value) == '{0}: line {1}: {2}'.format(src, n_head + line, sc.TEXT[kind]), name
        assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')


def test_header_errors(tmp_path):
    dst = str(tmp_path / 'out.bam')
    for header, what in (('@HD\tVN:1.6\n', 'no @SQ line in the header'), ('', 'no @SQ line in the header'),
                         ('@HD\tVN:1.6\n@SQ\tSN:c1\tLN:10\n@SQ\tLN:10\n', 'line 3: @SQ line without SN'),
                         ('@SQ\tSN:c1\n', 'line 1: @SQ line without LN'), ('@SQ\tSN:c1\tLN:ten\n', 'line 1: @SQ line whose LN is not an integer below 2^31'),
                         ('@SQ\tSN:c1\tLN:2147483648\n', 'line 1: @SQ line whose LN is not an integer below 2^31')):
        src = sc.write_sam(str(tmp_path / 'h.sam'), sc.VALID['one'], header)
        with pytest.raises(ValueError) as e:
            bam.sam_to_bam(src, dst)
        assert str(e.value) == '{0}: {1}'.format(src, what)
        assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')
    # a header and no alignment line is a valid file of no records; @SQ lines keep their order and their other fields
    header = '@SQ\tSN:zz\tLN:7\tM5:abc\n@SQ\tLN:9\tSN:aa\n@CO\tfree text\n'
    src = sc.write_sam(str(tmp_path / 'only_header.sam'), b'', header)
    bam.sam_to_bam(src, dst)
    assert bam.read_header(dst) == [('zz', 7), ('aa', 9)] and inflate_file(dst) == sc.bam_header(header, [('zz', 7), ('aa', 9)])


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({'ref': rng.choice([0, 1, -1], n, p=[0.6, 0.3, 0.1]), 'pos': rng.integers(0, 90000, n),
                         'qname': ['r{0}'.format(i) for i in range(n)],
                         'cigar': rng.choice(['50M', '20M100N30M', '5S40M5S', '10M2I10M1D18M', '7M'], n),
                         'flag': rng.choice([0, 16, 4], n), 'nh': rng.choice([1, 2], n), 'nh_type': rng.choice(list('cCsSiI'), n)})


def test_fixture_rows_round_trip_on_the_host(tmp_path):
    """The rows of _bam_fixtures as SAM text, converted, sorted and indexed by the host builds: the sorted file holds the rows'
    names, places, flags and CIGARs in the order the fixture's writer gives them, and the same bases and qualities."""
    expect_rows = _rows(700, 5)
    expect_rows.loc[expect_rows.ref < 0, 'pos'] = -1
    expect_rows = bf.sort_reads(expect_rows)
    lines = sc.sam_text(expect_rows, sc.REFS, seed=3).split(b'\n')[:-1]
    order = sc.shuffled_order(expect_rows, 9)
    text = b''.join(lines[k] + b'\n' for k in order)
    assert sc.encode(text)[1].size == len(expect_rows) + 1
    src = sc.write_sam(str(tmp_path / 'x.sam'), text)
    conv, srt = bam.sam_to_bam(src, str(tmp_path / 'x.bam'), window_bytes=20000), str(tmp_path / 'x_sorted.bam')
    assert bam.sort_order(conv) == 'unsorted'
    bam.sort_bam(conv, srt)
    bam.create_index(srt)
    assert bam.sort_order(srt) == 'coordinate' and bam.verify_bgzf(srt)['blocks'] >= 2
    expect, expect_off = bf.encode_records(expect_rows, seed=3)
    data = inflate_file(srt)
    data = data[bam.parse_header(data)[0]:]
    off, used, _ = bam.frame_records(data)
    assert used == len(data) and len(off) == len(expect_rows)
    for k, (o, e) in enumerate(zip(off.tolist(), expect_off.tolist())):
        got, want = data[o:], expect[e:]
        l_name, n_cig, l_seq = got[12], struct.unpack_from('<H', got, 16)[0], struct.unpack_from('<i', got, 20)[0]
        assert got[4:13] == want[4:13] and got[16:32] == want[16:32], k          # refID, pos, l_read_name; n_cigar_op .. next_pos
        body = 36 + l_name + 4 * n_cig
        assert got[36:body] == want[36:body], k                                 # name and CIGAR
        assert got[body:body + l_seq // 2] == want[body:body + l_seq // 2], k   # bases (the spare nibble of an odd length apart)
        q = body + (l_seq + 1) // 2
        assert got[q:q + l_seq] == want[q:q + l_seq], k                         # qualities
    index = bam.parse_bai(srt + '.bai')
    assert index.tobytes() == bam.build_index(srt).tobytes() and len(index.refs) == len(sc.REFS)


def test_command_line_checks(tmp_path):
    from degnorm_amd import __main__ as cli
    gtf = os.path.join(ROOT, 'tests', 'golden', 'pipeline.gtf')
    sams = [sc.write_sam(str(tmp_path / (s + '.sam')), sc.VALID['one']) for s in ('a', 'b')]
    other = str(tmp_path / 'other')
    os.makedirs(other)
    twin = sc.write_sam(os.path.join(other, 'a.sam'), sc.VALID['one'])
    bam_file = sc.write_sam(str(tmp_path / 'x.bam'), b'')

    def check(*argv):
        return cli.validate_args(cli.argparser().parse_args(list(argv) + ['-g', gtf]))

    ok = check('--sam-files', *sams)
    assert ok.sam_files == sams and ok.bam_files == [] and ok.bai_files == [] and ok.sort_bam_files == [] and ok.create_bai_files == []
    assert check('--sam-dir', str(tmp_path), '--native-deflate', '-p', '2').sam_files == sams
    for argv, exc, text in ((['--sam-files'] + sams + ['--bam-files', bam_file, bam_file], ValueError, 'together with --bam-files'),
                            (['--sam-files'] + sams + ['--bam-dir', str(tmp_path)], ValueError, 'together with --bam-files'),
                            (['--sam-files'] + sams + ['--bai-files', 'x.bai'], ValueError, 'together with --bam-files'),
                            (['--sam-files'] + sams + ['-w', str(tmp_path)], ValueError, 'together with --bam-files'),
                            (['--sam-files'] + sams + ['--sam-dir', str(tmp_path)], ValueError, 'both --sam-files and --sam-dir'),
                            (['--sam-files', sams[0]], ValueError, 'Fewer than 2 .sam files'),
                            (['--sam-files', sams[0], bam_file], ValueError, 'x.bam is not a .sam file.'),
                            (['--sam-files', sams[0], str(tmp_path / 'none.sam')], FileNotFoundError, 'none.sam'),
                            (['--sam-files', sams[0], twin], ValueError, 'not uniquely named'),
                            (['--sam-dir', other], ValueError, 'Only found 1 .sam files'),
                            (['--sam-dir', str(tmp_path / 'nowhere')], NotADirectoryError, 'nowhere')):
        with pytest.raises(exc) as e:
            check(*argv)
        assert text in str(e.value), argv
    # what the .bam flags say of a .sam file has not changed
    with pytest.raises(ValueError, match='a.sam is not a .bam file.'):
        check('--bam-files', *sams)
    with pytest.raises(ValueError, match='must have a .bam extension'):
        utils.sort_bam_file(sams[0])
    text = cli.argparser().format_help()
    assert '--sam-files' in text and '--sam-dir' in text and 'converted_bam' in text
