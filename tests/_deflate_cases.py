"""
Inputs and judges for the tests of the library's DEFLATE encoder (degnorm_amd.bam.bgzf_deflate, csrc/dn_deflate.hip); numpy,
struct and zlib only, the library is never called here.

    parts()          {case name: [bytes, ...]} -- every case of the host tests; built once, read only
    many_parts()     3 000 parts of 300 bytes
    judge(part, blk) the BGZF block `blk` holds `part`: header, BSIZE, a raw-DEFLATE payload zlib inflates to the part, CRC32
                     and ISIZE, and is no larger than stored_bound
    stored_bound(n)  the largest block n input bytes may become
    resolved(index, path)  a BamIndex with its virtual offsets replaced by offsets into the inflated file
"""
import struct
import zlib

import numpy as np

BLOCK_DATA = 0xff00
CUT = 8192                         # input bytes of one DEFLATE block (csrc/dn_deflate.hip kCut; DESIGN.md "BGZF deflate")
HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')
PSEUDO_BIN = 37450
_PARTS = {}


def stored_bound(n):
    return n + 26 + 6 * max(1, -(-n // CUT))


def judge(part, blk):
    assert blk[:16] == HEAD and len(blk) <= 65536
    assert struct.unpack_from('<H', blk, 16)[0] == len(blk) - 1
    assert zlib.decompress(blk[18:-8], -15) == part
    assert struct.unpack_from('<II', blk, len(blk) - 8) == (zlib.crc32(part) & 0xffffffff, len(part))
    assert len(blk) <= stored_bound(len(part))


def de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) (Lyndon words), as a list of letters 0 .. k - 1."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def fibonacci_counts(n=22):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _random(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def pipeline_parts():
    """The record streams of the three pipeline samples, cut into blocks as sort_bam cuts them."""
    import _bam_fixtures as bf
    import _gtf_fixtures as gf
    from degnorm_amd.bam import _block_cuts
    out = []
    for k in range(len(gf.PIPELINE_SAMPLES)):
        data, offs = bf.encode_records(gf.pipeline_bam_rows(k))
        ends = np.append(offs[1:], len(data)).astype(np.int64)
        out.append([data[a:b] for a, b in _block_cuts([ends])])
    return out


def parts():
    if _PARTS:
        return _PARTS
    rng = np.random.default_rng(1951)
    _PARTS['tiny'] = [b'', b'a', b'ab', b'abc', b'abcd', b'abcde']
    _PARTS['one_byte'] = [b'\x07' * BLOCK_DATA]
    seq = de_bruijn(4, 3)
    _PARTS['de_bruijn'] = [bytes(b'ACGT'[c] for c in seq + seq[:2])]
    assert len(_PARTS['de_bruijn'][0]) == 66
    _PARTS['random'] = [_random(rng, BLOCK_DATA)]
    _PARTS['chunk'] = [(_random(rng, 1000) * 66)[:BLOCK_DATA]]
    far = _random(rng, 32768)
    _PARTS['distance'] = [far + far[:BLOCK_DATA - 32768], far + b'\x00' + far[:BLOCK_DATA - 32769]]
    counts = fibonacci_counts()
    assert sum(counts) == 46367
    skew = np.repeat(rng.permutation(256)[:22].astype(np.uint8), counts)
    _PARTS['skewed'] = [rng.permutation(skew).tobytes()]
    # a period of 101 bytes: once the first period is out, matches of 258 bytes follow one another; none starts at a
    # multiple of 64 (101 + 258 k is odd), so one lies across every step boundary and every DEFLATE-block cut, and the
    # last ends with the input
    _PARTS['straddle'] = [(_random(rng, 101) * 260)[:101 + 258 * 100]]
    for k, blocks in enumerate(pipeline_parts()):
        _PARTS['pipeline{0}'.format(k)] = blocks
    return _PARTS


def many_parts():
    data = b''.join(pipeline_parts()[0])
    return [data[150 * k:150 * k + 300] for k in range(3000)]


def resolved(index, path):
    """
    The content of a BamIndex of the BGZF file `path` with every virtual offset (compressed offset of a block << 16 | offset
    in the block) replaced by the offset of the byte it names in the inflated file: what two files that hold the same
    blocks' data, deflated by different encoders, agree on.
    """
    from degnorm_amd.bam import bgzf_blocks
    offs, _, isizes = bgzf_blocks(path)
    start = dict(zip(offs.tolist(), (np.cumsum(isizes) - isizes).tolist()))

    def at(v):
        v = int(v)
        return start[v >> 16] + (v & 0xffff)
    out = []
    for ref in index.refs:
        bins = []
        for bin_id, ch in ref['bins']:
            flat = [int(x) for x in np.asarray(ch).reshape(-1)]
            if bin_id == PSEUDO_BIN:
                bins.append((bin_id, [at(flat[0]), at(flat[1])] + flat[2:]))
            else:
                bins.append((bin_id, [at(x) for x in flat]))
        out.append((bins, [at(x) for x in ref['ioffset']]))
    return out, index.n_no_coor
