"""
Inputs of the BGZF inflate tests (test_inflate_host.py, test_gpu_inflate.py), built with Python's zlib only: valid raw-deflate
payloads of every kind the decoder must handle, seeded corruptions of them, zlib's verdict on a payload, and a guarded call
of the library's host decoder.
"""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bam_fixtures as bf                                     # noqa: E402

FULL = 65280                                                    # the data bytes of a full BGZF block (0xff00)
GUARD = 64
SYNC_MARKER = b'\x00\x00\xff\xff'                               # the empty stored block a flush appends


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def bgzf(payload, isize, crc=0):
    """A whole BGZF block around a raw-deflate payload (the CRC32 is not checked by any reader here)."""
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', len(payload) + 25) + payload +
            struct.pack('<II', crc, isize))


def zlib_verdict(payload):
    """What zlib makes of a raw-deflate payload: its output when the stream ends exactly with the payload, else None."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


def _text(rng, n):
    words = [b'coverage', b'degradation', b'transcript', b'exon', b'read', b'chr1', b'gene_name', b'\t', b'\n', b' ', b'0123', b'+', b';']
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(len(words)))]
        if rng.random() < 0.05:
            out += bytes(rng.integers(32, 127, size=int(rng.integers(1, 12)), dtype=np.uint8))
    return bytes(out[:n])


def _bam_records(seed, n):
    rng = np.random.default_rng(seed)
    k = 700
    pos = np.sort(rng.integers(0, 1 << 20, size=k))
    cig = rng.choice(['100M', '40M2000N60M', '5S95M', '50M1I49M', '30M1D70M'], k)
    df = pd.DataFrame({'ref': 0, 'pos': pos, 'qname': ['read.{0}'.format(i) for i in range(k)], 'cigar': cig, 'nh': 1, 'nh_type': 'C'})
    return bf.encode_records(df, seed)[0][:n]


def data_kinds(seed=0):
    """(name, bytes): the data every level is tried on."""
    rng = np.random.default_rng(seed)
    half = bytes(rng.integers(0, 256, size=FULL // 2, dtype=np.uint8))
    return [('text', _text(rng, FULL)), ('bam', _bam_records(seed, FULL)), ('zeros', bytes(FULL)), ('run', b'\x5a' * FULL),
            ('random', bytes(rng.integers(0, 256, size=FULL, dtype=np.uint8))), ('far', half + half)]


def flushed_stream(seed=1):
    """(data, payload, the payload offsets just after each mid-stream flush): a sync and a full flush in the middle."""
    rng = np.random.default_rng(seed)
    parts = [_text(rng, 9000), _bam_records(seed, 14000), _text(rng, 7000)]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(parts[0]) + c.flush(zlib.Z_SYNC_FLUSH)
    marks = [len(payload)]
    payload += c.compress(parts[1]) + c.flush(zlib.Z_FULL_FLUSH)
    marks.append(len(payload))
    payload += c.compress(parts[2]) + c.flush()
    return b''.join(parts), payload, marks


def valid_cases(seed=0):
    """(name, data, payload) of every valid case; the payload is raw deflate, data what it must inflate to."""
    cases = []
    kinds = data_kinds(seed)
    for level in (0, 1, 6, 9):
        for name, data in kinds:
            cases.append(('{0}-l{1}'.format(name, level), data, deflate(data, level)))
    for sname, strategy in (('fixed', zlib.Z_FIXED), ('huffman', zlib.Z_HUFFMAN_ONLY), ('rle', zlib.Z_RLE)):
        for name, data in kinds[:4]:
            cases.append(('{0}-{1}'.format(name, sname), data, deflate(data, 6, strategy)))
    rng = np.random.default_rng(seed + 1)
    for n in (0, 1, 2, 3):
        data = bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
        for level in (0, 1, 6):
            cases.append(('tiny{0}-l{1}'.format(n, level), data, deflate(data, level)))
    near = bytes(rng.integers(0, 256, size=32500, dtype=np.uint8))                 # zlib's own matches reach back 32506 at most
    cases.append(('near-l9', near + near, deflate(near + near, 9)))
    head = bytes(rng.integers(0, 256, size=32768, dtype=np.uint8))                 # by hand: length 258 at distance 32768
    w = _Bits()
    w.put(0, 3)
    w.put(0, 5)
    w.put(32768, 16)
    w.put(32767, 16)
    w.acc |= int.from_bytes(head, 'little') << w.n
    w.n += 8 * len(head)
    w.put(1, 1)
    w.put(1, 2)
    w.code(0xc5, 8)
    w.code(29, 5)
    w.put(8191, 13)
    w.code(0, 7)
    cases.append(('dist-max', head + head[:258], w.bytes()))
    cases.append(('eof', b'', b'\x03\x00'))                                     # the payload of BGZF's end-of-file block
    data, payload, _ = flushed_stream(seed + 2)
    cases.append(('flushes', data, payload))
    a, b = _text(rng, 20000), _bam_records(seed + 3, 20000)                        # two streams joined: the first ends in a flush
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    cases.append(('joined', a + b, c.compress(a) + c.flush(zlib.Z_FULL_FLUSH) + deflate(b, 1)))
    return cases


def blocks_of(cases):
    return [bgzf(p, len(d), zlib.crc32(d)) for _, d, p in cases]


class _Bits(object):
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):                    # a field, least significant bit first
        self.acc |= value << self.n
        self.n += nbits

    def code(self, value, nbits):                   # a Huffman code, most significant bit first
        for k in range(nbits - 1, -1, -1):
            self.put((value >> k) & 1, 1)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, 'little')


_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _canonical(lens):
    """{(code length, code): symbol} of a canonical Huffman code."""
    code, out = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                out[(n, code)] = s
                code += 1
        code <<= 1
    return out


def deflate_block_types(payload):
    """
    The BTYPE of every deflate block of a valid raw-deflate payload, in order: a bit-level walk that decodes the symbols of the
    Huffman blocks only to find where each one ends (nothing is written).
    """
    acc, pos, types = int.from_bytes(payload, 'little'), 0, []

    def take(n):
        nonlocal pos
        v = (acc >> pos) & ((1 << n) - 1)
        pos += n
        return v

    def symbol(table):
        code = 0
        for n in range(1, 16):
            code = code << 1 | take(1)
            if (n, code) in table:
                return table[(n, code)]
        raise ValueError('no such code')

    last = 0
    while not last:
        last, kind = take(1), take(2)
        types.append(kind)
        if kind == 0:
            pos = (pos + 7) & ~7
            pos += 32 + 8 * (take(16) & 0xffff)
            continue
        if kind == 1:
            lit, dist = _canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _canonical([5] * 30)
        else:
            n_lit, n_dist, n_cl = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(n_cl):
                cl[_CL_ORDER[k]] = take(3)
            cl, lens = _canonical(cl), []
            while len(lens) < n_lit + n_dist:
                s = symbol(cl)
                lens += [s] if s < 16 else [lens[-1]] * (3 + take(2)) if s == 16 else [0] * (3 + take(3)) if s == 17 else [0] * (11 + take(7))
            lit, dist = _canonical(lens[:n_lit]), _canonical(lens[n_lit:])
        while True:
            s = symbol(lit)
            if s == 256:
                break
            if s > 256:
                take(0 if s < 265 or s == 285 else (s - 261) >> 2)
                d = symbol(dist)
                take(0 if d < 4 else (d - 2) >> 1)
    assert (pos + 7) >> 3 == len(payload)
    return types


def dynamic_header(cl_lens, lit_lens, dist_lens):
    """
    A final dynamic block's header.  cl_lens: the 19 lengths of the code-length code.  lit_lens / dist_lens: values 0 .. 3,
    written with two bits each -- right when cl_lens gives symbols 0 .. 3 two bits each, which is what the callers pass
    whenever the code-length code itself is not the thing under test.
    """
    w = _Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(15, 4)
    for s in _CL_ORDER:
        w.put(cl_lens[s], 3)
    for v in list(lit_lens) + list(dist_lens):
        w.code(v, 2)
    return w


def crafted():
    """(kind, payload, isize) of hand-made streams; `ok-lone` is valid, the others must be refused."""
    two = [2, 2, 2, 2] + [0] * 15
    out = []
    lit = [0] * 257
    lit[65], lit[256] = 1, 1                                    # 'A' = 0, end of block = 1
    w = dynamic_header(two, lit, [0])
    for _ in range(5):
        w.code(0, 1)
    w.code(1, 1)
    out.append(('ok-lone', w.bytes(), 5))
    out.append(('cl-oversubscribed', dynamic_header([1] * 19, lit, [0]).bytes() + bytes(40), 5))
    out.append(('cl-incomplete', dynamic_header([2] + [0] * 18, lit, [0]).bytes() + bytes(40), 5))
    over = [0] * 257
    over[0], over[1], over[2], over[256] = 1, 1, 1, 1
    out.append(('lit-oversubscribed', dynamic_header(two, over, [0]).bytes() + bytes(40), 5))
    inc = [0] * 257
    inc[0], inc[256] = 2, 2
    out.append(('lit-incomplete', dynamic_header(two, inc, [0]).bytes() + bytes(40), 5))
    out.append(('dist-oversubscribed', dynamic_header(two, lit, [1, 1, 1]).bytes() + bytes(40), 5))
    out.append(('dist-incomplete', dynamic_header(two, lit, [2, 2, 0]).bytes() + bytes(40), 5))
    noeob = [0] * 257
    noeob[65], noeob[66] = 1, 1
    out.append(('no-end-of-block', dynamic_header(two, noeob, [0]).bytes() + bytes(40), 5))
    w = _Bits()                                                  # fixed block whose first symbol is a match of 3 at distance 1
    w.put(1, 1)
    w.put(1, 2)
    w.code(1, 7)
    w.code(0, 5)
    w.code(0, 7)
    out.append(('match-first', w.bytes(), 3))
    w = _Bits()
    w.put(1, 1)
    w.put(3, 2)
    out.append(('type-3', w.bytes() + bytes(8), 0))
    return out


def mutations(seed=0, n_flips=900, n_cuts=600, n_trailing=300, n_stored=200):
    """(kind, payload, isize): seeded corruptions of valid payloads, most of which no decoder may accept."""
    rng = np.random.default_rng(seed)
    pool = [(d, p) for name, d, p in valid_cases(seed) if len(p) > 8]
    small = [(d[:3000], deflate(d[:3000], lv)) for lv in (1, 6, 9) for _, d in data_kinds(seed)[:2]]
    pool += small
    coded = [(d, p) for d, p in pool if len(p) < 0.9 * len(d)]                  # Huffman-coded: a flipped bit is not just data
    out = []
    for k in range(n_flips):
        d, p = coded[int(rng.integers(len(coded)))]
        q = bytearray(p)
        bit = int(rng.integers(8 * min(len(q), 40))) if k % 4 else int(rng.integers(8 * len(q)))     # most of them in the block header
        q[bit >> 3] ^= 1 << (bit & 7)
        out.append(('flip', bytes(q), len(d)))
    d, p = small[3]
    for cut in range(64):
        out.append(('cut', p[:cut], len(d)))
    for _ in range(n_cuts):
        d, p = pool[int(rng.integers(len(pool)))]
        out.append(('cut', p[:int(rng.integers(len(p)))], len(d)))
    for d, p in pool[::2]:
        for isize in (len(d) - 1, len(d) + 1, 0, 65536):
            if 0 <= isize <= 65536 and isize != len(d):
                out.append(('isize', p, isize))
    stored = [(d, deflate(d, 0)) for _, d in data_kinds(seed)] + [(d[:100], deflate(d[:100], 0)) for _, d in data_kinds(seed)]
    for _ in range(n_stored):
        d, p = stored[int(rng.integers(len(stored)))]
        q = bytearray(p)
        bit = int(rng.integers(32))                                                # LEN / NLEN of the first stored block
        q[1 + (bit >> 3)] ^= 1 << (bit & 7)
        out.append(('stored', bytes(q), len(d)))
    for _ in range(n_trailing):
        d, p = pool[int(rng.integers(len(pool)))]
        out.append(('trailing', p + bytes(rng.integers(0, 256, size=int(rng.integers(1, 5)), dtype=np.uint8)), len(d)))
    out += [c for c in crafted() if c[0] != 'ok-lone']
    return out


def host_inflate(payload, isize):
    """
    dn_bgzf_inflate_host on one payload, its input and output surrounded by guard bytes: (return code, status, output).
    Asserts that the guards are untouched.
    """
    from degnorm_amd import _lib
    lib = _lib.load()
    comp = np.full(len(payload) + 2 * GUARD, 0xa5, np.uint8)
    comp[GUARD:GUARD + len(payload)] = np.frombuffer(payload, np.uint8)
    out = np.full(max(isize, 0) + 2 * GUARD, 0xa5, np.uint8)
    pay_off, pay_len = np.array([0], np.int64), np.array([len(payload)], np.int32)
    out_off, status = np.array([0, isize], np.int64), np.array([-99], np.int32)
    P, c = ctypes.POINTER, ctypes
    rc = lib.dn_bgzf_inflate_host(c.cast(comp.ctypes.data + GUARD, P(c.c_uint8)), len(payload), 1, pay_off.ctypes.data_as(P(c.c_int64)),
                                  pay_len.ctypes.data_as(P(c.c_int32)), out_off.ctypes.data_as(P(c.c_int64)),
                                  c.cast(out.ctypes.data + GUARD, P(c.c_uint8)), status.ctypes.data_as(P(c.c_int32)))
    assert (out[:GUARD] == 0xa5).all() and (out[len(out) - GUARD:] == 0xa5).all(), 'the decoder wrote outside out'
    assert (comp[:GUARD] == 0xa5).all() and (comp[len(comp) - GUARD:] == 0xa5).all()
    return rc, int(status[0]), out[GUARD:GUARD + max(isize, 0)].tobytes()
