"""
Cases and the definition for the tests of degnorm_amd.bam.sort_bam (numpy, pandas, struct and zlib only; the library is
never called here).

    build_case(name, path)      write case `name` -- an unsorted BAM file -- to path; returns what the checks need
    spec_sorted(stream, n_ref)  the definition of include/degnorm_amd.h in plain Python: parse the inflated records, sort
                                their ordinals by (ref_key, pos + 1) with Python's stable sort, concatenate
    inflate_file(path)          (inflated bytes, inflated size of every block, the file's bytes) of a BGZF file, by zlib
    error_files(tmp)            {name: (path, keywords, text the ValueError must contain)} of the files sort_bam refuses

Rows are encoded in the order given (_bam_fixtures.encode_records); the header text says SO:unsorted, SO:queryname or has
no @HD line.
"""
import struct
import zlib

import numpy as np
import pandas as pd

import _bai_cases as bc
import _bam_fixtures as bf

WINDOWS = (None, 4096, 1)
SEGMENTS = (None, 256)
BLOCK_DATA = 0xff00
HD_OUT = '@HD\tVN:1.6\tSO:coordinate\n'
HEADERS = {'unsorted': ('@HD\tVN:1.6\tSO:unsorted\n', HD_OUT),
           'queryname': ('@HD\tVN:1.5\tSO:queryname\tGO:query\n', '@HD\tVN:1.5\tSO:coordinate\tGO:query\n'),
           'none': ('', HD_OUT)}
REFS = [('chrA', 300000), ('chrE', 1000), ('chrB', 200000)]


def header_pair(refs, form, extra=''):
    """The header bytes of an input with header `form` and of its sorted output; extra: @CO lines behind the @SQ lines."""
    sq = ''.join('@SQ\tSN:{0}\tLN:{1}\n'.format(nm, ln) for nm, ln in refs) + extra
    tail = struct.pack('<i', len(refs))
    for nm, ln in refs:
        b = nm.encode() + b'\x00'
        tail += struct.pack('<i', len(b)) + b + struct.pack('<i', ln)
    out = []
    for hd in HEADERS[form]:
        t = (hd + sq).encode()
        out.append(b'BAM\x01' + struct.pack('<i', len(t)) + t + tail)
    return out[0], out[1]


def _rows(ref, pos, cigar='50M', flag=0):
    return pd.DataFrame({'ref': ref, 'pos': pos, 'cigar': cigar, 'flag': flag})


def _named(parts, order=None, seed=0):
    df = pd.concat(parts, ignore_index=True)
    df['qname'] = ['q{0}'.format(k) for k in range(len(df))]
    if order == 'scramble':
        df = df.iloc[np.random.default_rng(seed).permutation(len(df))]
    elif order == 'sorted':
        df = bf.sort_reads(df)
    elif order == 'reversed':
        df = bf.sort_reads(df).iloc[::-1]
    return df.reset_index(drop=True)


def _placed(rng, n=1200):
    parts = []
    for ref, length, k in ((0, 300000, n), (2, 200000, n // 2)):
        parts.append(_rows(ref, rng.integers(0, length - 400, k), rng.choice(['50M', '20M300N30M', '10S40M', '25M2I23M'], k).tolist()))
        parts.append(_rows(ref, rng.integers(0, length - 400, 40), None, 4))          # unmapped mates with coordinates
    return parts


def case_three():
    rng = np.random.default_rng(1)
    return REFS, _named(_placed(rng) + [_rows(-1, np.full(120, -1), None, 4)], 'scramble', 1), 'unsorted', 'aligned'


def case_ties():
    """Runs of 40 .. 200 records of one (refID, pos), scrambled: the stability case."""
    rng = np.random.default_rng(2)
    parts = [_rows(int(r), np.full(int(k), int(p)), '50M') for r, p, k in
             zip(rng.choice([0, 2], 24), rng.integers(0, 30, 24) * 1000, rng.integers(40, 200, 24))]
    return REFS, _named(parts + [_rows(-1, np.full(60, -1), None, 4)], 'scramble', 2), 'queryname', 'aligned'


def case_sorted():
    return REFS, _named(_placed(np.random.default_rng(3)) + [_rows(-1, np.full(50, -1), None, 4)], 'sorted'), 'none', 'aligned'


def case_reversed():
    return REFS, _named(_placed(np.random.default_rng(4)) + [_rows(-1, np.full(50, -1), None, 4)], 'reversed'), 'unsorted', 'aligned'


def case_unplaced():
    return REFS, _named([_rows(-1, np.full(900, -1), None, 4)]), 'queryname', 'aligned'


def case_empty():
    return REFS, _named([_rows(0, [], '50M')]), 'unsorted', 'aligned'


def case_minus_one():
    """pos -1 on placed records: they lead their reference."""
    rng = np.random.default_rng(5)
    parts = _placed(rng, 400) + [_rows(0, [-1, -1, 0], ['50M', None, '50M'], [0, 4, 0]), _rows(2, [-1], '50M')]
    return REFS, _named(parts, 'scramble', 5), 'none', 'aligned'


def case_long():
    """Two records of 105 kB, longer than a BGZF block holds, among ordinary ones."""
    rng = np.random.default_rng(6)
    parts = _placed(rng, 300) + [_rows(0, [150000, 10], '70000M'), _rows(-1, np.full(20, -1), None, 4)]
    return REFS, _named(parts, 'scramble', 6), 'unsorted', 'straddle'


def case_straddle():
    rng = np.random.default_rng(7)
    return REFS, _named(_placed(rng) + [_rows(-1, np.full(80, -1), None, 4)], 'scramble', 7), 'queryname', 'straddle'


def case_midheader():
    rng = np.random.default_rng(8)
    return REFS, _named(_placed(rng, 500) + [_rows(-1, np.full(30, -1), None, 4)], 'scramble', 8), 'none', 'midheader'


CASES = {'three': case_three, 'ties': case_ties, 'sorted': case_sorted, 'reversed': case_reversed, 'unplaced': case_unplaced,
         'empty': case_empty, 'minus_one': case_minus_one, 'long': case_long, 'straddle': case_straddle, 'midheader': case_midheader}
# 'three' has an empty reference in the middle (chrE) and unplaced reads


def build_case(name, path, level=1):
    """Write case `name` to path.  Returns {'refs', 'rows', 'stream' (the records as written), 'header_in', 'header_out'}."""
    refs, rows, form, layout = CASES[name]()
    data, offs = bf.encode_records(rows)
    hdr_in, hdr_out = header_pair(refs, form, '@CO\tkept as it is\n')
    if len(rows):
        cuts = bc.layout_cuts(layout, len(hdr_in), offs, len(data))
    else:
        cuts = []
    bc.write_layout(path, hdr_in, data, cuts, level)
    return {'refs': refs, 'rows': rows, 'stream': data, 'header_in': hdr_in, 'header_out': hdr_out}


def parse_records(stream):
    """(start, end, refID, pos) of every record of an inflated record stream."""
    out, o = [], 0
    while o < len(stream):
        bs, ref, pos = struct.unpack_from('<iii', stream, o)
        assert bs >= 32 and o + 4 + bs <= len(stream)
        out.append((o, o + 4 + bs, ref, pos))
        o += 4 + bs
    return out


def spec_sorted(stream):
    """The sorted record stream by the definition, and the ends of its records."""
    recs = parse_records(stream)
    order = sorted(range(len(recs)), key=lambda k: (0xffffffff if recs[k][2] == -1 else recs[k][2], recs[k][3] + 1))
    ends = np.cumsum([recs[k][1] - recs[k][0] for k in order]).astype(np.int64) if recs else np.zeros(0, np.int64)
    return b''.join(stream[recs[k][0]:recs[k][1]] for k in order), ends


def inflate_file(path):
    """(inflated bytes, [inflated size of each block], the file's bytes) of a BGZF file; every block's CRC32 and ISIZE are checked."""
    raw = open(path, 'rb').read()
    p, out, sizes = 0, [], []
    while p < len(raw):
        assert raw[p:p + 4] == b'\x1f\x8b\x08\x04' and raw[p + 12:p + 16] == b'BC\x02\x00'
        total = struct.unpack_from('<H', raw, p + 16)[0] + 1
        data = zlib.decompress(raw[p + 18:p + total - 8], -15)
        crc, isize = struct.unpack_from('<II', raw, p + total - 8)
        assert isize == len(data) and crc == zlib.crc32(data) & 0xffffffff
        out.append(data)
        sizes.append(len(data))
        p += total
    return b''.join(out), sizes, raw


def check_layout(path, header_out, ends):
    """The block rules of a written file: EOF block, at most 0xff00 bytes a block, blocks start where a record starts."""
    data, sizes, raw = inflate_file(path)
    assert raw.endswith(bf.EOF_BLOCK) and sizes[-1] == 0
    assert max(sizes) <= BLOCK_DATA
    starts = np.concatenate([[0], np.cumsum(sizes[:-1])])
    bounds = np.concatenate([[0, len(header_out)], len(header_out) + ends])
    rec_len = np.diff(bounds)
    for s in starts.tolist():
        k = int(np.searchsorted(bounds, s, side='right')) - 1
        if bounds[k] != s:
            assert k < len(rec_len) and rec_len[k] > BLOCK_DATA, 'a block starts inside record {0}, which fits a block'.format(k - 1)
            assert (s - bounds[k]) % BLOCK_DATA == 0
    return data


def error_files(tmp):
    refs = [('chrA', 100000), ('chrB', 100000)]
    hdr = header_pair(refs, 'unsorted')[0]
    rng = np.random.default_rng(9)
    n = 1200
    good = _rows(rng.choice([0, 1], n), rng.integers(0, 90000, n), '50M')
    good['qname'] = ['q{0}'.format(k) for k in range(n)]
    out = {}

    def write(name, frame, text, kw=None, eof=True, level=1, patch=None, raw_patch=None):
        data, offs = bf.encode_records(frame.reset_index(drop=True))
        if patch:
            data = patch(bytearray(data), offs)
        p = str(tmp / (name + '.bam'))
        blocks = bc.write_layout(p, hdr, bytes(data), bc.layout_cuts('straddle', len(hdr), offs, len(data)), level, eof=eof)
        if raw_patch:
            raw = bytearray(open(p, 'rb').read())
            raw_patch(raw, blocks)
            open(p, 'wb').write(bytes(raw))
            text = text.format(blocks[3][0])
        out[name] = (p, kw or {}, text)

    def small_block_size(data, offs):
        data[offs[700]:offs[700] + 4] = struct.pack('<i', 20)
        small_block_size.at = int(offs[700])
        return data

    def bad_type(raw, blocks):
        raw[blocks[3][0] + 18] = 0x07                       # final block of the reserved type 3

    def flip(raw, blocks):
        raw[blocks[3][0] + 18 + 5 + 200] ^= 0x10            # a stored block (level 0): the data changes, the block still inflates

    write('no_eof', good, 'no BGZF end-of-file block', eof=False)
    write('inflate', good, 'the BGZF block at byte {0} does not inflate: bad block type or header', raw_patch=bad_type)
    write('crc', good, 'the BGZF block at byte {0} does not inflate: CRC32 differs from the block trailer', kw={'verify': True}, level=0,
          raw_patch=flip)
    write('block_size', good, None, patch=small_block_size)
    out['block_size'] = out['block_size'][:2] + ('malformed BAM record 700 at byte {0} of the record stream: block_size 20 is below 32'
                                                 .format(small_block_size.at),)
    bad = good.copy()
    bad.loc[800, 'ref'] = 2
    write('ref_range', bad, 'record 800 (refID 2, position {0}) names a reference the header does not have (2 references)'.format(int(bad.pos[800])))
    bad = good.copy()
    bad.loc[300, 'pos'] = -7
    write('pos_range', bad, 'record 300 (refID {0}, position -7) has a position below -1'.format(int(bad.ref[300])))

    def many_cigar_ops(data, offs):                         # n_cigar_op; block_size stays, so the chain of records is intact
        data[offs[700] + 16:offs[700] + 18] = struct.pack('<H', 0xffff)
        return data

    # the two texts below are what the library gave before the index and the sort shared their error path
    write('shape', good, 'malformed BAM record 700 (refID 1, position 35368): its read name and CIGAR do not fit inside the record', patch=many_cigar_ops)
    bad = good.copy()                                       # the earlier fault has the larger code: the ordinal decides
    bad.loc[300, 'pos'] = -7
    bad.loc[900, 'ref'] = 2
    write('two_faults', bad, 'record 300 (refID 1, position -7) has a position below -1')
    return out
