"""
Cases and an independent builder for the tests of degnorm_amd.bam.build_index (numpy, pandas, struct and zlib only; the
library is never called here).

    spec_index(refs, records, blocks)   the canonical .bai of include/degnorm_amd.h, record by record, in plain Python
    spec_query(bai, tid, beg, end)      the reader of the SAM specification 5.3 on the bytes of a .bai
    write_layout(path, hdr, data, cuts, level)   a BGZF writer that cuts the stream (header + records) wherever told

records: (sorted reads frame, start of every record in the stream, stream length); blocks: (file offset, stream start,
size) of every block, the end-of-file block included.
"""
import struct

import numpy as np
import pandas as pd

import _bam_fixtures as bf

PSEUDO = 37450
REF_OPS = set('MDN=X')
WINDOWS = (1, 70000, None)
SEGMENTS = (256, None)
LAYOUTS = ('aligned', 'straddle', 'midheader', 'empty')
# the sizes every error file is built with: one window; a window per block; windows of four blocks, so that a fault at record
# 900 of an error file lies in a later window and its text must still count the records of the windows before
ERROR_SIZES = ({}, {'window_bytes': 1, 'segment_bytes': 256}, {'window_bytes': 70000})
BLOCK = 20000


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += list(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def span(ref, pos, flag, cigar):
    """[beg, end) of a record as the index sees it."""
    rlen, num = 0, ''
    for ch in cigar if isinstance(cigar, str) else '':
        if ch.isdigit():
            num += ch
        else:
            rlen += int(num) if ch in REF_OPS else 0
            num = ''
    if flag & 4 or not isinstance(cigar, str) or not cigar or rlen == 0:
        rlen = 1
    beg, end = pos, pos + rlen
    if ref >= 0:
        beg, end = max(beg, 0), (1 if end <= 0 else end)
    return beg, end


def voffset(blocks, u):
    """The virtual offset of stream position u."""
    last = None
    for k, (coff, start, size) in enumerate(blocks):
        if size > 0:
            last = k
            if start <= u < start + size:
                return coff << 16 | (u - start)
    assert u == blocks[last][1] + blocks[last][2]
    return blocks[last + 1][0] << 16


def record_table(records):
    """(ref, beg, end, flag, stream start, stream end) of every record."""
    reads, starts, total = records
    flags = reads['flag'].tolist() if 'flag' in reads else [0] * len(reads)
    ends = list(starts[1:]) + [total]
    out = []
    for k, (ref, pos, cigar) in enumerate(zip(reads['ref'].tolist(), reads['pos'].tolist(), reads['cigar'].tolist())):
        beg, end = span(int(ref), int(pos), int(flags[k]), cigar)
        out.append((int(ref), beg, end, int(flags[k]), int(starts[k]), int(ends[k])))
    return out


def spec_index(refs, records, blocks):
    n_ref = len(refs)
    bins = [dict() for _ in range(n_ref)]            # bin -> chunks in file order
    lin = [dict() for _ in range(n_ref)]
    meta = [None] * n_ref                            # [first vbeg, last vend, mapped, unmapped]
    n_no_coor, prev = 0, None
    for ref, beg, end, flag, s, e in record_table(records):
        vb, ve = voffset(blocks, s), voffset(blocks, e)
        if ref < 0:
            n_no_coor += 1
            prev = None
            continue
        assert beg <= 1 << 29 and end <= 1 << 29
        b = reg2bin(beg, end)
        if prev == (ref, b):
            bins[ref][b][-1][1] = ve
        else:
            bins[ref].setdefault(b, []).append([vb, ve])
        prev = (ref, b)
        if meta[ref] is None:
            meta[ref] = [vb, ve, 0, 0]
        meta[ref][1] = ve
        meta[ref][3 if flag & 4 else 2] += 1
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[ref][w] = min(lin[ref].get(w, vb), vb)
    out = bytearray(b'BAI\x01' + struct.pack('<i', n_ref))
    for r in range(n_ref):
        if meta[r] is None:
            out += struct.pack('<ii', 0, 0)
            continue
        out += struct.pack('<i', len(bins[r]) + 1)
        for b in sorted(bins[r]):
            merged = []
            for vb, ve in bins[r][b]:
                if merged and merged[-1][1] >> 16 >= vb >> 16:
                    merged[-1][1] = ve
                else:
                    merged.append([vb, ve])
            out += struct.pack('<Ii', b, len(merged))
            for vb, ve in merged:
                out += struct.pack('<QQ', vb, ve)
        out += struct.pack('<Ii', PSEUDO, 2) + struct.pack('<QQQQ', *meta[r])
        n_intv = 1 + max(lin[r])
        io = [None] * n_intv
        for w in range(n_intv - 1, -1, -1):
            io[w] = lin[r][w] if w in lin[r] else io[w + 1]
        out += struct.pack('<i', n_intv) + struct.pack('<{0}Q'.format(n_intv), *io)
    out += struct.pack('<Q', n_no_coor)
    return bytes(out)


def spec_query(bai, tid, beg, end):
    """The chunks to scan for [beg, end) of reference tid, from the bytes of a .bai (SAM specification 5.3)."""
    p = 8
    for r in range(tid + 1):
        n_bin = struct.unpack_from('<i', bai, p)[0]
        p += 4
        chunks = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from('<Ii', bai, p)
            p += 8
            chunks[b] = [struct.unpack_from('<QQ', bai, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
        n_intv = struct.unpack_from('<i', bai, p)[0]
        io = struct.unpack_from('<{0}Q'.format(n_intv), bai, p + 4)
        p += 4 + 8 * n_intv
    low = io[min(beg >> 14, n_intv - 1)] if n_intv else 0
    cand = sorted(c for b in reg2bins(beg, end) for c in chunks.get(b, []) if c[1] > low)
    out = []
    for vb, ve in cand:
        if out and vb <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], ve))
        else:
            out.append((vb, ve))
    return out


def write_layout(path, hdr, data, cuts, level, eof=True):
    """
    Write hdr + data as BGZF blocks cut at the stream positions `cuts` (0 and the end are implied; a position given twice
    makes an empty block there).  Returns the (file offset, stream start, size) of every block.
    """
    stream = hdr + data
    edges = [0] + sorted(c for c in cuts if 0 < c < len(stream)) + [len(stream)]
    out, blocks = bytearray(), []
    for a, b in zip(edges[:-1], edges[1:]):
        assert b - a <= 0xff00
        blocks.append((len(out), a, b - a))
        out += bf._bgzf_block(stream[a:b], level)
    if eof:
        blocks.append((len(out), len(stream), 0))
        out += bf.EOF_BLOCK
    with open(path, 'wb') as f:
        f.write(bytes(out))
    return blocks


def layout_cuts(layout, n_hdr, offs, n_data):
    """The cuts of one of LAYOUTS, for a header of n_hdr bytes and records starting at offs (within the data)."""
    if layout == 'straddle':                         # every BLOCK bytes of the stream: the header ends inside a block
        return list(range(BLOCK, n_hdr + n_data, BLOCK))
    cuts, last = [], -BLOCK
    for o in offs.tolist():                          # at record starts: every block ends where a record ends
        if o - last >= BLOCK - 300:
            cuts.append(n_hdr + o)
            last = o
    if layout == 'midheader':                        # the header spans three blocks and ends inside the third
        return [10, 50] + cuts[1:]
    if layout == 'empty':                            # an empty block in the middle of the file and one behind the header
        return cuts + [cuts[0], cuts[len(cuts) // 2]]
    return cuts


def _frame(ref, pos, cigar, flag=0):
    return pd.DataFrame({'ref': ref, 'pos': pos, 'cigar': cigar, 'flag': flag})


def _finish(parts):
    df = pd.concat(parts, ignore_index=True)
    df['qname'] = ['q{0}'.format(k) for k in range(len(df))]
    return bf.sort_reads(df)


def case_three():
    """Three references, the middle one empty, a tail of unplaced reads; unmapped, CIGAR-less, I / S-only reads, pos -1."""
    rng = np.random.default_rng(5)
    refs = [('chrA', 300000), ('chrE', 1000), ('chrB', 200000)]
    parts = []
    for ref, length, n in ((0, 300000, 1700), (2, 200000, 1200)):
        pos = np.sort(rng.integers(0, length - 400, n))
        cig = rng.choice(['50M', '20M300N30M', '10S40M', '25M2I23M', '30M5D20M', '40=10X'], n).tolist()
        parts.append(_frame(ref, pos, cig))
        parts.append(_frame(ref, rng.integers(0, length - 400, 60), None, 4))                # unmapped mates with coordinates
        parts.append(_frame(ref, rng.integers(0, length - 400, 40), None, 0))                # no CIGAR
        parts.append(_frame(ref, rng.integers(0, length - 400, 40), '20S30I', 0))            # no reference base
        parts.append(_frame(ref, [-1, -1], ['50M', None], [0, 4]))
        parts.append(_frame(ref, np.full(300, 16384 * 3 + 100), '50M'))                       # a long run of one bin
    parts.append(_frame(-1, np.full(150, -1), None, 4))
    return refs, _finish(parts)


def case_deep():
    """A reference of 2^29 bases with spliced reads of 40 kb and 70 Mb: all six bin levels, claims of many windows."""
    rng = np.random.default_rng(6)
    L = 1 << 29
    refs = [('chrL', L), ('chrS', 100000)]
    n = 2400
    pos = rng.integers(0, L - 80_000_000, n)
    cig = rng.choice(['50M', '50M', '25M40000N25M', '20M500000N30M', '30M5000000N20M'], n).tolist()
    parts = [_frame(0, pos, cig)]
    parts.append(_frame(0, rng.integers(0, L - 80_000_000, 12), '25M70000000N25M'))
    parts.append(_frame(0, [L - 50, L - 1], ['50M', '1M']))                                   # ends at 2^29 exactly
    parts.append(_frame(0, np.full(400, 5 << 20) + np.arange(400) % 7, '50M'))                # a long run of one bin
    parts.append(_frame(0, rng.integers(0, L - 1000, 30), None, 4))
    parts.append(_frame(1, np.sort(rng.integers(0, 99000, 500)), '50M'))
    return refs, _finish(parts)


CASES = {'three': case_three, 'deep': case_deep}


def build_case(name, layout, path, level=1):
    """Write case `name` in `layout` to path.  Returns (refs, records, blocks, sorted reads)."""
    refs, reads = CASES[name]()
    data, offs = bf.encode_records(reads)
    hdr = bf.header_bytes(refs)
    blocks = write_layout(path, hdr, data, layout_cuts(layout, len(hdr), offs, len(data)), level)
    return refs, (reads, offs + len(hdr), len(hdr) + len(data)), blocks, reads


def regions(refs, reads, n, seed):
    """n seeded (tid, beg, end) on references that have reads, of every scale."""
    rng = np.random.default_rng(seed)
    tids = sorted(set(int(r) for r in reads['ref'] if r >= 0))
    out = []
    for _ in range(n):
        tid = int(rng.choice(tids))
        length = refs[tid][1]
        size = int(rng.choice([1, 100, 20000, 300000, 5_000_000, 100_000_000]))
        beg = int(rng.integers(0, length))
        out.append((tid, beg, min(beg + size, length)))
    return out


def error_files(tmp):
    """{name: (path, text the ValueError must contain)} of the files build_index refuses."""
    refs = [('chrA', 100000), ('chrB', 1 << 29)]
    hdr = bf.header_bytes(refs)
    rng = np.random.default_rng(9)
    n = 1200
    good = _frame(0, np.sort(rng.integers(0, 90000, n)), '50M')
    good['qname'] = ['q{0}'.format(k) for k in range(n)]
    out = {}

    def write(name, frame, text, hdr=hdr, cut=0, eof=True, corrupt=False, patch=None):
        data, offs = bf.encode_records(frame.reset_index(drop=True))
        if patch:
            data = bytes(patch(bytearray(data), offs))
        if cut:
            data = data[:-cut]
        p = str(tmp / (name + '.bam'))
        blocks = write_layout(p, hdr, data, layout_cuts('straddle', len(hdr), offs, len(data)), 1, eof=eof)
        if corrupt:
            raw = bytearray(open(p, 'rb').read())
            raw[blocks[3][0] + 18] = 0x07                    # final block of the reserved type 3
            open(p, 'wb').write(bytes(raw))
            text = text.format(blocks[3][0])
        out[name] = (p, text)

    bad = good.copy()
    bad.loc[700, 'ref'] = 1
    write('ref_order', bad, 'not sorted by coordinate: record 701 (refID 0')
    bad = good.copy()
    bad.loc[900, 'pos'] = 5
    write('pos_order', bad, 'not sorted by coordinate: record 900 (refID 0, position 5)')
    assert len(hdr) + bf.encode_records(good)[1][900] > 4 * BLOCK       # behind the first window of ERROR_SIZES[2]: four blocks
    bad = good.copy()
    bad.loc[n - 1, 'ref'] = 2
    write('ref_range', bad, 'record {0} (refID 2'.format(n - 1))
    bad = pd.concat([good, _frame(1, [(1 << 29) - 10], '50M').assign(qname='far')])
    write('beyond', bad, 'record {0} (refID 1, position {1}) reaches beyond position 2^29'.format(n, (1 << 29) - 10))
    write('cut', good, 'record {0} is cut by the end of the file'.format(n - 1), cut=10)
    write('no_eof', good, 'no BGZF end-of-file block', eof=False)
    write('inflate', good, 'the BGZF block at byte {0} does not inflate: bad block type or header', corrupt=True)

    def many_cigar_ops(data, offs):                          # n_cigar_op; block_size stays, so the chain of records is intact
        data[offs[700] + 16:offs[700] + 18] = struct.pack('<H', 0xffff)
        return data

    # the three texts below are what the library gave before the index and the sort shared their error path
    write('shape', good, 'malformed BAM record 700 (refID 0, position 54355): its read name and CIGAR do not fit inside the record', patch=many_cigar_ops)
    bad = good.copy()                                        # the earlier fault has the larger code: the ordinal decides
    bad.loc[300, 'pos'] = 5
    bad.loc[900, 'ref'] = 2
    write('two_faults', bad, 'BAM file is not sorted by coordinate: record 300 (refID 0, position 5) follows a larger position of the same reference')
    return out
