"""
gzip files for the gz tests (test tooling, not product code), and a plain-Python restatement of the "gzip streams" section of
include/degnorm_amd.h that shares no code with the product: a bit-by-bit inflate that lists the block boundaries, the guess
rule, the segment table and the marker propagation.  Everything is seeded; the compressor is Python's own zlib.
"""
import gzip
import os
import struct
import tempfile
import zlib

import numpy as np

import _gtf_fixtures as gf

HIST = 32768
# zlib closes a block after 16 383 symbols, and on this text a symbol stands for about 30 bytes: a text of 400 KB is one final block,
# which no rule can guess.  1.3 MB gives every level several blocks and the restatement still takes about a second a case.
TEXT_BYTES = 1300000
CHUNKS = (4096, 16384, 1 << 20)
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# --- builders -------------------------------------------------------------------------------------------------------------------

def gtf_text(min_bytes, seed=24):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 't.gtf')
        gf.write_gtf(path, seed, min_bytes)
        with open(path, 'rb') as f:
            return f.read()


def raw_deflate(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, sync_every=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if sync_every is None:
        return co.compress(plain) + co.flush()
    parts = []
    for lo in range(0, len(plain), sync_every):
        parts.append(co.compress(plain[lo:lo + sync_every]))
        parts.append(co.flush(zlib.Z_SYNC_FLUSH))
    return b''.join(parts) + co.flush()


def member(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, sync_every=None, extra=None, name=None, comment=None, hcrc=False, deflated=None):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = b'\x1f\x8b\x08' + bytes([flg]) + b'\0\0\0\0\0\xff'
    if extra is not None:
        head += struct.pack('<H', len(extra)) + extra
    if name is not None:
        head += name + b'\0'
    if comment is not None:
        head += comment + b'\0'
    if hcrc:
        head += struct.pack('<H', zlib.crc32(head) & 0xffff)
    body = raw_deflate(plain, level, strategy, sync_every) if deflated is None else deflated
    return head + body + struct.pack('<II', zlib.crc32(plain) & 0xffffffff, len(plain) & 0xffffffff)


_CASES = None


def cases():
    """{name: (gzip bytes, plain bytes)}; built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(24)
    text = gtf_text(TEXT_BYTES)
    small = text[:150000]
    c = {}
    for level in (1, 6, 9):
        c['text{0}'.format(level)] = (member(text, level), text)
    c['fixed'] = (member(small, 6, zlib.Z_FIXED), small)
    c['huffman_only'] = (member(small, 6, zlib.Z_HUFFMAN_ONLY), small)
    c['rle'] = (member(small, 6, zlib.Z_RLE), small)
    c['stored'] = (member(small, 0), small)
    c['empty'] = (member(b''), b'')
    c['one_byte'] = (member(b'x'), b'x')
    c['m32768'] = (member(text[:32768]), text[:32768])
    c['m32769'] = (member(text[:32769]), text[:32769])
    block = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    c['long_refs'] = (member(block * 6, 6), block * 6)
    run = b'\0' * (1 << 20)
    c['run'] = (member(run, 0), run)                      # stored blocks of 65 535 bytes: each spans sixteen 4 KiB chunks
    run6 = b'A' * (1 << 20)
    c['run6'] = (member(run6, 6), run6)                   # references at distance 1, length 258
    c['sync_flush'] = (member(text, 6, sync_every=50000), text)
    c['nested'] = (member(c['text6'][0], 0), c['text6'][0])
    three = [small[:70000], b'', small[70000:]]
    c['three_members'] = (b''.join(member(p) for p in three), small)
    c['header_fields'] = (member(small, 6, extra=b'AB\x03\x00xyz', name=b'genes.gtf', comment=b'seeded', hcrc=True), small)
    c['zero_padding'] = (member(small) + b'\0' * 300, small)
    _CASES = c
    return c


def mutations(data, n, seed, first):
    """n seeded single-byte mutations of data at or behind byte `first`: (position, new byte) pairs."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(first, len(data), n)
    val = rng.integers(1, 256, n)
    return [(int(p), (data[int(p)] + int(v)) & 0xff) for p, v in zip(pos, val)]


# --- the restatement --------------------------------------------------------------------------------------------------------------

class Bad(Exception):
    pass


class Reader(object):
    def __init__(self, data, pos):
        self.d, self.p, self.n = data, pos, 8 * len(data)

    def bit(self):
        p = self.p
        if p >= self.n:
            raise Bad('input')
        self.p = p + 1
        return (self.d[p >> 3] >> (p & 7)) & 1

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v


def kraft(lengths):
    """The sum of 2^-len over the non-zero lengths, in units of 2^-15."""
    return sum(1 << (15 - l) for l in lengths if l)


def canonical(lengths):
    """{(length, code): symbol} of RFC 1951's canonical code."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def symbol(rd, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | rd.bit()
        s = table.get((l, code))
        if s is not None:
            return s
    raise Bad('code')


def dynamic_header(rd):
    """(literal/length lengths, distance lengths, code-length code lengths) of the dynamic block whose HLIT starts at rd."""
    hlit, hdist, hclen = rd.bits(5), rd.bits(5), rd.bits(4)
    if hlit > 29 or hdist > 29:
        raise Bad('header')
    cl = [0] * 19
    for i in range(hclen + 4):
        cl[_ORDER[i]] = rd.bits(3)
    table = canonical(cl)
    n, lens = hlit + 257 + hdist + 1, []
    while len(lens) < n:
        s = symbol(rd, table)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Bad('lengths')
            v, rep = lens[-1], 3 + rd.bits(2)
        elif s == 17:
            v, rep = 0, 3 + rd.bits(3)
        else:
            v, rep = 0, 11 + rd.bits(7)
        if len(lens) + rep > n:
            raise Bad('lengths')
        lens.extend([v] * rep)
    if lens[256] == 0:
        raise Bad('lengths')
    return lens[:hlit + 257], lens[hlit + 257:], cl


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
              16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST = [5] * 32


def block_symbols(rd, lit, dist, out):
    """The symbols of a block up to its end-of-block code; out (a list, or None) takes the symbols, references resolved."""
    while True:
        s = symbol(rd, lit)
        if s < 256:
            if out is not None:
                out.append(s)
        elif s == 256:
            return
        else:
            s -= 257
            if s >= 29:
                raise Bad('code')
            n = _LEN_BASE[s] + rd.bits(_LEN_EXTRA[s])
            d = symbol(rd, dist)
            if d >= 30:
                raise Bad('code')
            d = _DIST_BASE[d] + rd.bits(_DIST_EXTRA[d])
            if out is not None:
                if d > len(out):
                    raise Bad('distance')
                for _ in range(n):
                    out.append(out[-d])


def block(rd, out):
    """One block at rd into out; True when it was the final one."""
    final, kind = rd.bit(), rd.bits(2)
    if kind == 3:
        raise Bad('header')
    if kind == 0:
        rd.p = (rd.p + 7) & ~7
        n, m = rd.bits(16), rd.bits(16)
        if n ^ m != 0xffff:
            raise Bad('header')
        q = rd.p >> 3
        if q + n > len(rd.d):
            raise Bad('input')
        if out is not None:
            out.extend(rd.d[q:q + n])
        rd.p += 8 * n
    elif kind == 1:
        block_symbols(rd, canonical(_FIXED_LIT), canonical(_FIXED_DIST), out)
    else:
        ll, dl, _ = dynamic_header(rd)
        block_symbols(rd, canonical(ll), canonical(dl), out)
    return bool(final)


def passes(data, b):
    """The guess rule at bit b."""
    try:
        rd = Reader(data, b)
        if rd.bits(3) != 4:                                   # BFINAL = 0, BTYPE = 2
            return False
        ll, dl, cl = dynamic_header(rd)                         # rule 1 (HLIT, HDIST) and rule 3
        if kraft(cl) != 1 << 15:                                # rule 2
            return False
        if kraft(ll) != 1 << 15:                                # rule 4
            return False
        codes = [l for l in dl if l]
        if not (kraft(dl) == 1 << 15 or not codes or codes == [1]):
            return False
        block_symbols(rd, canonical(ll), canonical(dl), None)   # rule 5
        return rd.bits(3) >> 1 != 3                             # rule 6
    except Bad:
        return False


def candidates(data):
    """The bit offsets that pass rules 1 and 2 (the numpy form of them), ascending."""
    n = 8 * len(data)
    bits = np.concatenate([np.unpackbits(np.frombuffer(data, np.uint8), bitorder='little'), np.zeros(96, np.uint8)])
    idx = np.arange(n, dtype=np.int64)
    c = idx[(bits[:n] == 0) & (bits[1:n + 1] == 0) & (bits[2:n + 2] == 1)]

    def field(off, width):
        return sum(bits[c + off + i].astype(np.int64) << i for i in range(width))
    c = c[(field(3, 5) <= 29) & (field(8, 5) <= 29)]
    ncl = field(13, 4) + 4
    c, ncl = c[17 + 3 * ncl <= n - c], ncl[17 + 3 * ncl <= n - c]
    total = np.zeros(c.size, np.int64)
    for i in range(19):
        l = field(17 + 3 * i, 3)
        total += np.where((i < ncl) & (l > 0), 128 >> l, 0)
    return c[total == 128]


class Restated(object):
    """A gzip file by the definition: members, blocks, plain bytes; guess(C), segments(C), by_markers(C)."""

    def __init__(self, data):
        self.data = data
        self.blocks = []          # (first bit, end bit, final, output length, member)
        self.first = []           # the first block's bit of every member
        plain = []
        p, m = 0, 0
        while p < len(data):
            if m and data[p] == 0:
                p += 1
                continue
            assert data[p:p + 3] == b'\x1f\x8b\x08'
            flg = data[p + 3]
            q = p + 10
            if flg & 4:
                q += 2 + struct.unpack_from('<H', data, q)[0]
            for f in (8, 16):
                if flg & f:
                    q = data.index(b'\0', q) + 1
            if flg & 2:
                q += 2
            rd, out = Reader(data, 8 * q), []
            self.first.append(rd.p)
            while True:
                a, n0 = rd.p, len(out)
                final = block(rd, out)
                self.blocks.append((a, rd.p, final, len(out) - n0, m))
                if final:
                    break
            plain.append(bytes(out))
            p = ((rd.p + 7) >> 3) + 8
            m += 1
        self.members = m
        self.plain = b''.join(plain)
        self._cand = None
        self._pass = {}

    def guess(self, C):
        if self._cand is None:
            self._cand = candidates(self.data)
        n_chunks = (len(self.data) + C - 1) // C
        g = np.full(n_chunks, -1, np.int64)
        cut = np.searchsorted(self._cand, np.arange(n_chunks + 1, dtype=np.int64) * 8 * C)
        for k in range(n_chunks):
            for b in self._cand[cut[k]:cut[k + 1]].tolist():
                if b not in self._pass:
                    self._pass[b] = passes(self.data, b)
                if self._pass[b]:
                    g[k] = b
                    break
        return g

    def segments(self, C, stats=None):
        """(entry, exit, out_len, kind) rows in chain order; stats: confirmed, jumped, fixups, segments, blocks."""
        g = self.guess(C)
        rows, k = [], 0
        st = dict(confirmed=0, jumped=0, fixups=0)
        while k < len(self.blocks):
            entry, c, n = self.blocks[k][0], self.blocks[k][0] // (8 * C), 0
            confirmed = g[c] == entry
            st['confirmed' if confirmed else 'fixups'] += 1
            while True:
                _, end, final, out_len, _ = self.blocks[k]
                n += out_len
                k += 1
                if final or (end >= 8 * (c + 1) * C if confirmed else g[end // (8 * C)] == end):
                    break
            rows.append((entry, end, n, 1 if final else 0))
            st['jumped'] += max(end // (8 * C) - c - 1, 0)
        st.update(segments=len(rows), blocks=len(self.blocks), members=self.members, chunks=len(g), guessed=int((g >= 0).sum()))
        if stats is not None:
            stats.update(st)
        return g, np.array(rows, np.int64).reshape(-1, 4)

    def by_markers(self, C):
        """The plain bytes by the marker scheme: every segment decoded without its history, windows propagated, markers resolved."""
        _, rows = self.segments(C)
        out, win = [], [0] * HIST
        for entry, exit_, n, kind in rows.tolist():
            if entry in self.first:
                win = [0] * HIST
            syms = list(range(0x8000, 0x8000 + HIST))
            rd = Reader(self.data, entry)
            while rd.p < exit_:
                block(rd, syms)
            assert rd.p == exit_ and len(syms) - HIST == n
            out.append(bytes(s if s < 256 else win[s & 0x7fff] for s in syms[HIST:]))
            tail = syms[-HIST:]
            win = [t if t < 256 else win[t & 0x7fff] for t in tail]
        return b''.join(out)


_RESTATED = {}


def restated(name):
    if name not in _RESTATED:
        _RESTATED[name] = Restated(cases()[name][0])
    return _RESTATED[name]


def reference(data):
    """gzip.decompress(data), or the exception it raises."""
    try:
        return gzip.decompress(data)
    except Exception as e:          # EOFError, zlib.error, gzip.BadGzipFile
        return e


# --- malformed files: (name, bytes, offset of the member the error names, what) ------------------------------------------------------

class _BitWriter(object):
    def __init__(self):
        self.bits = []

    def put(self, value, n):                    # n bits, least significant first (header fields, extra bits)
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, value, n):                   # a Huffman code, most significant bit first
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[8 * k + i] << i for i in range(8)) for k in range(len(b) // 8))


def far_reference():
    """A final fixed block whose first symbol is a reference: length 3, distance 5, with nothing before it."""
    w = _BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    w.code(0b0000001, 7)                        # length symbol 257: 3 bytes
    w.code(4, 5)                                # distance symbol 4: 5 .. 6, one extra bit
    w.put(0, 1)
    w.code(0, 7)                                # end of block
    return w.bytes()


def error_cases():
    z, text = cases()['text6']
    small = text[:20000]
    head = 10
    out = []
    cuts = [1, 5, 9, 10, 11, 12, len(z) // 2, len(z) - 9, len(z) - 8, len(z) - 4, len(z) - 1]
    for n in cuts:
        what = 'truncated header' if n < head else 'truncated deflate stream' if n <= len(z) - 9 else 'truncated trailer'
        out.append(('cut_at_{0}'.format(n), z[:n], 0, what))
    out.append(('bad_magic', b'\x1f\x8c' + z[2:], 0, 'bad magic'))
    out.append(('cm_7', z[:2] + b'\x07' + z[3:], 0, 'compression method 7'))
    out.append(('reserved_flag', z[:3] + b'\x20' + z[4:], 0, 'reserved flag bits set'))
    stored = bytearray(member(small, 0))
    stored[head + 5 + 7000] ^= 0x10
    out.append(('stored_bit_flip', bytes(stored), 0, 'CRC32 mismatch'))
    wrong = member(small)
    out.append(('wrong_isize', wrong[:-4] + struct.pack('<I', len(small) + 1), 0, 'ISIZE mismatch'))
    first = member(small)
    second = member(b'', deflated=far_reference())
    out.append(('reference_before_member', first + second, len(first), 'distance beyond the start of the member'))
    out.append(('trailing_garbage', z + b'\0\0garbage', len(z) + 2, 'trailing garbage'))
    fields = bytearray(member(small, hcrc=True, name=b'n'))
    fields[12] ^= 1
    out.append(('header_crc', bytes(fields), 0, 'header CRC mismatch'))
    # the next entry is bit 8 n of a file whose size n is a multiple of the chunk: no span can be formed behind it
    def pad(xlen):
        return b'AB' + struct.pack('<H', xlen - 4) + b'\0' * (xlen - 4)
    out.append(('header_ends_the_file', member(b'', extra=pad(4096 - 12), deflated=b'')[:-8], 0, 'truncated deflate stream'))
    first = member(small)
    second = member(b'', extra=pad(8192 - 12 - len(first) % 4096), deflated=b'')[:-8]
    assert (len(first) + len(second)) % 4096 == 0
    out.append(('second_header_ends_the_file', first + second, len(first), 'truncated deflate stream'))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    flushed = co.compress(text[:50000]) + co.flush(zlib.Z_SYNC_FLUSH)          # ends byte-aligned behind an empty stored block
    cut = member(b'', extra=pad(8192 - 12 - len(flushed) % 4096), deflated=flushed)[:-8]
    assert len(cut) % 4096 == 0
    out.append(('cut_behind_a_sync_flush', cut, 0, 'truncated deflate stream'))
    return out
