"""
gz.gunzip / gz.scan on the host build (no GPU): the bytes against Python's gzip, the tables and counters against the restatement
of include/degnorm_amd.h ("gzip streams") in _gz_cases.py, the errors with their offsets and texts, and seeded mutations.
"""
import gzip
import struct
import zlib

import numpy as np
import pytest

import _gz_cases as gc
from degnorm_amd import bam, gz

NAMES = sorted(gc.cases())
COUNTERS = ('members', 'chunks', 'guessed', 'confirmed', 'jumped', 'fixups', 'segments', 'blocks')


@pytest.mark.parametrize('name', NAMES)
def test_bytes_equal_gzip(name):
    z, plain = gc.cases()[name]
    assert gzip.decompress(z) == plain
    for chunk in gc.CHUNKS:
        st = {}
        assert gz.gunzip(z, chunk_bytes=chunk, stats=st) == plain, chunk
        assert st['bytes_in'] == len(z) and st['bytes_out'] == len(plain) and st['bgzf'] is False


@pytest.mark.parametrize('name', NAMES)
def test_tables_equal_the_restatement(name):
    z, _ = gc.cases()[name]
    r = gc.restated(name)
    assert r.plain == gc.cases()[name][1]
    for chunk in gc.CHUNKS:
        want, got = {}, {}
        guess_r, seg_r = r.segments(chunk, want)
        guess, seg = gz.scan(z, chunk_bytes=chunk, stats=got)
        np.testing.assert_array_equal(guess, guess_r)
        np.testing.assert_array_equal(seg, seg_r)
        assert {k: got[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}, chunk
        st = {}
        gz.gunzip(z, chunk_bytes=chunk, stats=st)
        assert {k: st[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}, chunk


@pytest.mark.parametrize('name', ['text1', 'long_refs', 'sync_flush', 'three_members', 'run6', 'm32769'])
def test_marker_scheme_gives_the_serial_bytes(name):
    assert gc.restated(name).by_markers(4096) == gc.cases()[name][1]


def _stats(name, chunk):
    st = {}
    gz.gunzip(gc.cases()[name][0], chunk_bytes=chunk, stats=st)
    return st


def test_counters_hold_where_the_cases_make_them():
    for name in ('text1', 'text6', 'text9'):
        assert _stats(name, 4096)['confirmed'] > 0, name
    assert _stats('run', 4096)['jumped'] > 0
    assert _stats('nested', 4096)['fixups'] > 0
    assert _stats('sync_flush', 4096)['fixups'] > 0
    st = _stats('fixed', 4096)
    assert st['guessed'] == 0 and st['segments'] == st['members'] == 1


@pytest.mark.parametrize('name', NAMES)
def test_spans_give_the_bytes_of_one_span(name):
    z, plain = gc.cases()[name]
    for chunk in (4096, 16384):
        assert gz.gunzip(z, chunk_bytes=chunk, window_bytes=65536) == plain, chunk


def test_bgzf_takes_the_block_path():
    _, text = gc.cases()['text6']
    text = text[:300000]
    z = b''.join(bam.bgzf_compress(text[lo:lo + 0xff00], 6) for lo in range(0, len(text), 0xff00)) + bam.BGZF_EOF
    st = {}
    assert gz.gunzip(z, stats=st) == text
    assert st['bgzf'] is True and st['bytes_out'] == len(text)
    assert gz.gunzip(z, window_bytes=65536) == text


ERRORS = gc.error_cases()


@pytest.mark.parametrize('case', ERRORS, ids=[e[0] for e in ERRORS])
def test_errors_name_member_and_cause(case):
    name, data, offset, what = case
    if what not in ('reserved flag bits set', 'header CRC mismatch'):       # Python's gzip looks at neither
        assert isinstance(gc.reference(data), Exception)
    for chunk, window in ((4096, None), (1 << 20, None), (4096, 65536)):
        with pytest.raises(ValueError) as e:
            gz.gunzip(data, chunk_bytes=chunk, window_bytes=window)
        assert str(e.value) == '<bytes>: gzip member at byte {0}: {1}'.format(offset, what)
    if what in ('CRC32 mismatch', 'header CRC mismatch'):
        assert len(gz.gunzip(data, verify=False)) == 20000
    else:
        with pytest.raises(ValueError):
            gz.gunzip(data, verify=False)


def test_errors_name_the_file(tmp_path):
    path = str(tmp_path / 'cut.gtf.gz')
    with open(path, 'wb') as f:
        f.write(gc.cases()['text6'][0][:-3])
    with pytest.raises(ValueError) as e:
        gz.gunzip(path)
    assert str(e.value) == path + ': gzip member at byte 0: truncated trailer'


def _structure(data):
    """The bytes of a one-member file with a ten-byte header whose CRC32 nobody compares, or the exception: zlib's raw inflate."""
    try:
        d = zlib.decompressobj(-15)
        out = d.decompress(data[10:])
        if not d.eof or len(d.unused_data) != 8:
            raise EOFError('truncated, or bytes behind the trailer')
        if struct.unpack('<I', d.unused_data[4:])[0] != len(out) & 0xffffffff:
            raise ValueError('ISIZE')
        return out
    except Exception as e:
        return e


def _mutate(data, first, n, seed):
    """Mutations that keep the structure: both decoders give the same bytes, and the CRC32 decides as it does in Python's gzip."""
    decoded = 0
    for pos, val in gc.mutations(data, n, seed, first):
        m = data[:pos] + bytes([val]) + data[pos + 1:]
        want = _structure(m)
        if isinstance(want, Exception):
            with pytest.raises(ValueError):
                gz.gunzip(m, chunk_bytes=4096, verify=False)
            continue
        decoded += 1
        assert gz.gunzip(m, chunk_bytes=4096, verify=False) == want, (pos, val)
        if isinstance(gc.reference(m), Exception):
            with pytest.raises(ValueError, match='CRC32 mismatch'):
                gz.gunzip(m, chunk_bytes=4096)
        else:
            assert gz.gunzip(m, chunk_bytes=4096) == want, (pos, val)
    return decoded


def test_mutations_raise_or_agree_with_zlib():
    decoded = _mutate(gc.cases()['text6'][0], 10, 2000, 6)
    if decoded == 0:
        _, text = gc.cases()['text6']
        decoded = _mutate(gc.member(text[:60000], 0), 10, 300, 7)
    assert decoded > 0


def test_open_text_reads_like_a_file(tmp_path):
    z, text = gc.cases()['three_members']
    path = str(tmp_path / 'x.gtf.gz')
    with open(path, 'wb') as f:
        f.write(z)
    with gz.open_text(path, chunk_bytes=4096, window_bytes=65536) as f:
        parts = []
        while True:
            more = f.read(7001)
            if not more:
                break
            parts.append(more)
    assert b''.join(parts) == text
    with gz.open_text(path) as f:
        assert f.read() == text
    plain = str(tmp_path / 'x.gtf')
    with open(plain, 'wb') as f:
        f.write(text)
    with gz.open_text(plain) as f:
        assert f.read() == text
    assert gz.inflated_size(path) == len(text)


def test_command_line_and_helper_take_sam_gz(tmp_path):
    """--sam-files and --sam-dir accept X.sam.gz, a directory with X.sam and X.sam.gz is refused with both names, and
    utils.sam_to_bam_file('X.sam.gz') writes X.bam with the bytes X.sam gives."""
    import os
    import _sam_cases as sc
    from degnorm_amd import __main__ as cli, utils
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gtf = os.path.join(root, 'tests', 'golden', 'pipeline.gtf')

    def zipped(path):
        with open(path, 'rb') as f, open(path + '.gz', 'wb') as g:
            g.write(gzip.compress(f.read()))
        os.remove(path)
        return path + '.gz'

    d = str(tmp_path / 'in')
    os.makedirs(d)
    a = zipped(sc.write_sam(os.path.join(d, 'a.sam'), sc.VALID['one']))
    b = sc.write_sam(os.path.join(d, 'b.sam'), sc.VALID['one'])

    def check(*argv):
        return cli.validate_args(cli.argparser().parse_args(list(argv) + ['-g', gtf]))

    assert check('--sam-files', a, b).sam_files == [a, b]
    assert check('--sam-dir', d).sam_files == [a, b]
    with pytest.raises(ValueError, match='is not a .sam file'):
        check('--sam-files', a, os.path.join(d, 'c.txt.gz'))
    with pytest.raises(ValueError, match='not uniquely named'):
        check('--sam-files', a, sc.write_sam(str(tmp_path / 'a.sam'), sc.VALID['one']))
    twin = sc.write_sam(os.path.join(d, 'a.sam'), sc.VALID['one'])
    with pytest.raises(ValueError) as e:
        check('--sam-dir', d)
    assert twin in str(e.value) and a in str(e.value)
    os.remove(twin)
    # the helper: X.sam.gz -> X.bam, the file X.sam gives
    plain = sc.write_sam(str(tmp_path / 'p.sam'), sc.VALID['one'] + sc.VALID['n257'])
    want = open(utils.sam_to_bam_file(plain), 'rb').read()
    os.remove(str(tmp_path / 'p.bam'))
    assert utils.sam_to_bam_file(zipped(plain)) == str(tmp_path / 'p.bam')
    assert open(str(tmp_path / 'p.bam'), 'rb').read() == want
    with pytest.raises(ValueError, match='must have a .sam extension'):
        utils.sam_to_bam_file(str(tmp_path / 'p.bam.gz'))
