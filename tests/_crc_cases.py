"""
Inputs of the BGZF CRC32 tests (test_crc_host.py, test_gpu_crc.py): blocks that every decoder accepts and whose bytes are
wrong all the same (found with zlib), the few hand-made ones, and a BAM file with one changed byte in a stored block.
"""
import functools
import os
import sys
import zlib

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bam_fixtures as bf                                     # noqa: E402
import _inflate_cases as ic                                    # noqa: E402

E_CRC = 8                                                       # DN_INFLATE_E_CRC
PER_CASE = 8


@functools.lru_cache(maxsize=None)
def silent_flips():
    """
    [(name, block)]: per kind ('text', 'bam') and coding (level 6, Z_FIXED) the first PER_CASE single-bit flips of the
    deflate payload that zlib still inflates to ISIZE bytes -- other bytes than the data.  The block's trailer holds the
    CRC32 of the true data, as a file damaged after it was written does.
    """
    out = []
    kinds = dict(ic.data_kinds()[:2])
    for kind in ('text', 'bam'):
        data = kinds[kind]
        for coding, strategy in (('l6', zlib.Z_DEFAULT_STRATEGY), ('fixed', zlib.Z_FIXED)):
            payload = ic.deflate(data, 6, strategy)
            found = 0
            for bit in range(8 * len(payload)):
                q = bytearray(payload)
                q[bit >> 3] ^= 1 << (bit & 7)
                got = ic.zlib_verdict(bytes(q))
                if got is not None and len(got) == len(data) and got != data:
                    out.append(('{0}-{1}-bit{2}'.format(kind, coding, bit), ic.bgzf(bytes(q), len(data), zlib.crc32(data))))
                    found += 1
                    if found == PER_CASE:
                        break
            assert found == PER_CASE, (kind, coding, found)
    return out


@functools.lru_cache(maxsize=None)
def handmade():
    """[(name, block, status the decoder must give with the check on)]."""
    data = dict(ic.data_kinds())['text'][:5000]
    stored = bytearray(ic.deflate(data, 0))
    stored[5 + 1234] ^= 0x20                                     # a stored block: 5 bytes of header, then the data verbatim
    good = ic.deflate(data, 6)
    cut = good[:len(good) // 2]                                  # does not decode, and its CRC32 is wrong as well
    rc, status, _ = ic.host_inflate(cut, len(data))
    assert rc == 0 and status not in (0, E_CRC)
    return [('stored-byte', ic.bgzf(bytes(stored), len(data), zlib.crc32(data)), E_CRC),
            ('crc-field-bit', ic.bgzf(good, len(data), zlib.crc32(data) ^ (1 << 17)), E_CRC),
            ('undecodable', ic.bgzf(cut, len(data), zlib.crc32(data) ^ 1), status)]


def host_statuses(blocks, verify=True):
    """The status of every block by the host build of the decoder (dn_bgzf_inflate_check_host), and the bytes of each."""
    import ctypes
    from degnorm_amd import _lib, bam
    comp, n_comp, pay_off, pay_len, isize = bam._block_layout(blocks)
    n = len(blocks)
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(isize[:n], out=out_off[1:])
    out, status = np.zeros(int(out_off[-1]) + 1, np.uint8), np.full(max(n, 1), -9, np.int32)
    P, c = ctypes.POINTER, ctypes
    crc = bam.block_crcs(blocks)
    rc = _lib.load().dn_bgzf_inflate_check_host(comp.ctypes.data_as(P(c.c_uint8)), n_comp, n, pay_off.ctypes.data_as(P(c.c_int64)),
                                                pay_len.ctypes.data_as(P(c.c_int32)), out_off.ctypes.data_as(P(c.c_int64)),
                                                out.ctypes.data_as(P(c.c_uint8)), status.ctypes.data_as(P(c.c_int32)),
                                                crc.ctypes.data_as(P(c.c_uint32)) if verify else None)
    assert rc == 0
    return status[:n], [out[out_off[k]:out_off[k + 1]].tobytes() for k in range(n)]


def damaged_bam(path):
    """
    Write a small single-end BAM of stored (level-0) blocks at path (with its index), then change one byte of an aux string
    in a block in the middle of the records.  Returns (chrom, offset of the damaged block, bytes of the undamaged file).
    """
    import _reads_fixtures as rf
    chrom, chrom_len, genes = rf.golden_layout()
    src = rf.synth_reads(31, (chrom, chrom_len, genes), 3000)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values})
    bf.write_bam(path, [(chrom, chrom_len)], df, block_size=20000, level=0)
    from degnorm_amd import bam
    offs, sizes, _ = bam.bgzf_blocks(path)
    with open(path, 'rb') as f:
        raw = bytearray(f.read())
    k = len(offs) // 2
    at = raw.index(b'hello world', int(offs[k]), int(offs[k] + sizes[k]))
    good = bytes(raw)
    raw[at + 4] = ord('0')                                       # 'hello world' -> 'hell0 world'
    with open(path, 'wb') as f:
        f.write(bytes(raw))
    return chrom, int(offs[k]), good


def crc_message(path, offset):
    return '{0}: the BGZF block at byte {1} does not inflate: CRC32 differs from the block trailer'.format(path, offset)
