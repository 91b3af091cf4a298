"""
A small BGZF / BAM / BAI writer for the tests of degnorm_amd.bam (numpy, struct and zlib only).

    write_bam(path, refs, reads, ...)   reads: DataFrame with `ref` (refID, -1 unplaced), `pos`, `qname`, `cigar` (a CIGAR
                                        string over MIDNSHP=X, '' or None for none) and optionally `next_ref`, `flag`,
                                        `nh` (None: no NH tag) and `nh_type` (the aux type letter NH is stored with)
                                        -> the record offsets of the inflated stream, in file order

Records are written sorted by (refID, pos), unplaced ones last.  Every record gets real seq / qual bytes and aux fields of
every type before and after NH.  With straddle=True the BGZF blocks are cut every block_size bytes of the inflated stream,
so records cross block boundaries; otherwise a block ends only at a record boundary (htslib's usual behaviour).  The
index holds, per reference, one real bin with one chunk and the pseudo-bin 37450, an empty linear index and n_no_coor.
"""
import struct
import zlib

import numpy as np

OPS = 'MIDNSHP=X'
EOF_BLOCK = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
_QUERY_OPS = {'M', 'I', 'S', '=', 'X'}


def _bgzf_block(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    bsize = 18 + len(raw) + 8 - 1
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', bsize) + raw +
            struct.pack('<II', zlib.crc32(data) & 0xffffffff, len(data)))


def _binary_cigar(cigar):
    """(packed uint32 ops, query length) of a CIGAR string."""
    ops, qlen, num = [], 0, ''
    for ch in cigar or '':
        if ch.isdigit():
            num += ch
        else:
            ops.append(int(num) << 4 | OPS.index(ch))
            qlen += int(num) if ch in _QUERY_OPS else 0
            num = ''
    return struct.pack('<{0}I'.format(len(ops)), *ops), len(ops), qlen


_PRE_AUX = (b'XAAx' + b'Xcc' + struct.pack('<b', -3) + b'XCC' + bytes([7]) + b'Xss' + struct.pack('<h', -300) +
            b'XSS' + struct.pack('<H', 60000) + b'Xii' + struct.pack('<i', -70000) + b'XII' + struct.pack('<I', 3000000000) +
            b'Xff' + struct.pack('<f', 1.5) + b'XZZhello world\x00' + b'XHH1AE301\x00' +
            b'XBBi' + struct.pack('<i', 3) + struct.pack('<3i', 1, 2, 3) + b'XbBc' + struct.pack('<i', 2) + b'\x01\x02')
_POST_AUX = b'ASC' + bytes([60]) + b'MDZ10A5\x00' + b'YBBf' + struct.pack('<i', 1) + struct.pack('<f', 0.25) + b'NMc\x00'


def nh_field(value, typ):
    """The NH aux field holding `value` as type `typ`."""
    fmt = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I', 'f': '<f'}
    if typ in fmt:
        return b'NH' + typ.encode() + struct.pack(fmt[typ], float(value) if typ == 'f' else int(value))
    if typ == 'A':
        return b'NHA' + str(value)[:1].encode()
    if typ == 'Z':
        return b'NHZ' + str(value).encode() + b'\x00'
    raise ValueError(typ)


def sort_reads(reads):
    """The rows in the order write_bam writes them (by refID, then pos; unplaced reads last; stable)."""
    ref = reads['ref'].values.astype(np.int64)
    key_ref = np.where(ref < 0, np.iinfo(np.int64).max, ref)
    o = np.lexsort((reads['pos'].values.astype(np.int64), key_ref))
    return reads.iloc[o].reset_index(drop=True)


def encode_records(reads, seed=0):
    """The BAM records of the (already sorted) rows as one bytes object and their start offsets."""
    rng = np.random.default_rng(seed)
    n = len(reads)
    qname = reads['qname'].astype(str).tolist()
    cig = reads['cigar'].tolist()
    ref = reads['ref'].values.astype(np.int64).tolist()
    pos = reads['pos'].values.astype(np.int64).tolist()
    nref = reads['next_ref'].values.astype(np.int64).tolist() if 'next_ref' in reads else [-1] * n
    flag = reads['flag'].values.astype(np.int64).tolist() if 'flag' in reads else [0] * n
    nh = reads['nh'].tolist() if 'nh' in reads else [None] * n
    nh_t = reads['nh_type'].tolist() if 'nh_type' in reads else ['C'] * n
    cig_cache, sq_cache = {}, {}
    recs, offs, o = [], np.zeros(n, dtype=np.int64), 0
    for k in range(n):
        c = cig[k] if isinstance(cig[k], str) else ''
        if c not in cig_cache:
            cig_cache[c] = _binary_cigar(c)
        cb, n_cig, l_seq = cig_cache[c]
        if l_seq not in sq_cache:
            sq_cache[l_seq] = (rng.integers(0, 256, size=(l_seq + 1) // 2, dtype=np.uint8).tobytes(),
                               rng.integers(2, 41, size=l_seq, dtype=np.uint8).tobytes())
        seq, qual = sq_cache[l_seq]
        name = qname[k].encode('ascii') + b'\x00'
        aux = _PRE_AUX + (nh_field(nh[k], nh_t[k]) if nh[k] is not None and nh[k] == nh[k] else b'') + _POST_AUX
        body = struct.pack('<iiBBHHHiiii', ref[k], pos[k], len(name), 60, 4680, n_cig, flag[k], l_seq, nref[k],
                           pos[k] if nref[k] >= 0 else -1, 0) + name + cb + seq + qual + aux
        recs.append(struct.pack('<i', len(body)) + body)
        offs[k] = o
        o += 4 + len(body)
    return b''.join(recs), offs


def header_bytes(refs, text='@HD\tVN:1.6\tSO:coordinate\n'):
    t = text + ''.join('@SQ\tSN:{0}\tLN:{1}\n'.format(nm, ln) for nm, ln in refs)
    out = b'BAM\x01' + struct.pack('<i', len(t)) + t.encode() + struct.pack('<i', len(refs))
    for nm, ln in refs:
        b = nm.encode() + b'\x00'
        out += struct.pack('<i', len(b)) + b + struct.pack('<i', ln)
    return out


def write_bam(path, refs, reads, straddle=False, block_size=0xff00, level=1, seed=0, index=True):
    """
    Write `reads` (sorted here, see sort_reads) as a BGZF BAM at path, and its index at path + '.bai' when index.
    Returns (sorted reads, record offsets in the inflated record stream, block starts of that stream).
    """
    reads = sort_reads(reads)
    data, offs = encode_records(reads, seed)
    hdr = header_bytes(refs)
    blocks, starts = [], []                    # starts: the inflated-stream offset of each record block
    if straddle:
        cuts = list(range(0, len(data), block_size))
    else:
        cuts, last = [], None
        for o in offs.tolist():
            if last is None or o - last >= block_size:
                cuts.append(o)
                last = o
        # a block may hold several records, and one record larger than block_size gets a block of its own
        if cuts and cuts[0] != 0:
            cuts.insert(0, 0)
    cuts = cuts + [len(data)]
    out = bytearray(_bgzf_block(hdr, level))
    coff = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b <= a:
            continue
        starts.append(a)
        coff.append(len(out))
        out += _bgzf_block(data[a:b], level)
    coff.append(len(out))
    starts.append(len(data))
    out += EOF_BLOCK
    with open(path, 'wb') as f:
        f.write(bytes(out))
    starts_a, coff_a = np.array(starts, dtype=np.int64), np.array(coff, dtype=np.int64)

    def voff(u):
        k = int(np.searchsorted(starts_a, u, side='right')) - 1
        return int(coff_a[k]) << 16 | int(u - starts_a[k])

    if index:
        ref = reads['ref'].values.astype(np.int64)
        unmapped = (reads['flag'].values.astype(np.int64) & 4) != 0 if 'flag' in reads else np.zeros(len(reads), bool)
        ends = np.append(offs[1:], len(data))
        bai = bytearray(b'BAI\x01' + struct.pack('<i', len(refs)))
        for t in range(len(refs)):
            rows = np.flatnonzero(ref == t)
            if rows.size == 0:
                bai += struct.pack('<i', 0) + struct.pack('<i', 0)
                continue
            beg, end = voff(int(offs[rows[0]])), voff(int(ends[rows[-1]]))
            n_unm = int(unmapped[rows].sum())
            bai += struct.pack('<i', 2)
            bai += struct.pack('<Ii', 4680, 1) + struct.pack('<QQ', beg, end)
            bai += struct.pack('<Ii', 37450, 2) + struct.pack('<QQQQ', beg, end, rows.size - n_unm, n_unm)
            bai += struct.pack('<i', 0)
        bai += struct.pack('<Q', int((ref < 0).sum()))
        with open(path + '.bai', 'wb') as f:
            f.write(bytes(bai))
    return reads, offs, starts_a
