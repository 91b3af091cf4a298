"""
Native BAM input for the reads stage: NativeBamReadsProcessor opens sorted, indexed .bam files without pysam.

    host      BGZF block walk; raw-deflate inflate (zlib, in a thread pool of n_jobs) of only the blocks that hold the
              requested chromosome, window by window (about window_bytes each; a record cut by a window end is carried to
              the next); the header's reference list; the .bai pseudo-bin of the chromosome; record framing in the
              library's host C++ (dn_bam_frame), which also checks that the range is sorted and belongs to the chromosome
              With inflate='device' the blocks of a window go to the device as they are in the file and the library's own
              DEFLATE decoder (csrc/dn_inflate.hip, one block per wavefront) builds the window where the decode kernels
              read it; the host frames a copy of it and uploads only the record offsets
              With frame='device' the window is framed where it lies (csrc/dn_frame.hip: every segment of the window guesses
              a record start and walks the block_size chain from it, the host stitches the per-segment table -- no window
              byte -- and has wrong guesses walked again, so the result is the serial walk's for every input).  Together
              with inflate='device' the inflated bytes never visit the host; the record cut by a window end waits on the
              device for the next window
    device    (csrc/dn_reads.hip) the records of each window are decoded, filtered by the reference's rules (reads.py
              load_chromosome_reads) and appended to a device-resident row store; the coverage stages read their binary
              CIGARs in place

Single-end reads never come back to the host.  Paired reads bring back only their qname_unpaired keys: the host sorts them
as pandas' sort_values does (numpy's quicksort on fixed-width bytes) and hands the order and the pair ids back.

A file without an index gets one from build_index / create_index (csrc/dn_bai.hip): one pass over every record of the file,
inflated, framed and indexed on the device window by window (or, device=None, with zlib and the host build of the same
source); parse_bai / BamIndex.tobytes / write_bai read and write whole .bai files, index_chunks is the region query.

A file that is not sorted by coordinate -- an aligner's default output -- is sorted by sort_bam (csrc/dn_sort.hip): the whole
inflated record stream is inflated into one device buffer, framed, keyed, radix-sorted (stably: ties keep file order) and
copied record by record into a second buffer; the host cuts, deflates (zlib) and writes the blocks of the sorted file under a
header that says SO:coordinate.  device=None does the same with zlib and the host build of the same source.  With
deflate='native' the blocks are written by the library's own DEFLATE encoder instead (csrc/dn_deflate.hip, bgzf_deflate): on the
device the sorted stream is deflated where it lies, one block per wavefront, and only the blocks come back.

Every path that inflates takes verify=True: the inflated bytes of each BGZF block are then compared with the CRC32 of its
trailer -- zlib.crc32 where zlib inflates, the wavefront that inflates the block where the device does -- and a block that
differs is a ValueError naming the file and the block's offset.  verify_bgzf checks a whole file that way (bgzip -t).
"""
import ctypes
import itertools
import os
import struct
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from ._lib import _check, _p as _ptr
from .reads import BamReadsProcessor, Annotation, coverage_outputs, reads_frame

BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
PSEUDO_BIN = 37450
CIGAR_OPS = 'MIDNSHP=X'
_INT32_MIN = -2 ** 31
_CHUNK = 4 << 20                 # compressed bytes read from the file at a time


# --- BGZF --------------------------------------------------------------------------------------------------------------

def _block_size(buf, p, where):
    """Total size of the BGZF block whose header starts at buf[p] (its BC extra subfield + 1)."""
    if buf[p:p + 4] != b'\x1f\x8b\x08\x04':
        raise ValueError('{0}: no BGZF block header at byte {1}'.format(where, p))
    xlen = struct.unpack_from('<H', buf, p + 10)[0]
    q, end = p + 12, p + 12 + xlen
    if end > len(buf):
        return None
    while q + 4 <= end:
        si1, si2, slen = buf[q], buf[q + 1], struct.unpack_from('<H', buf, q + 2)[0]
        if si1 == 66 and si2 == 67 and slen == 2:
            return struct.unpack_from('<H', buf, q + 4)[0] + 1
        q += 4 + slen
    raise ValueError('{0}: BGZF block at byte {1} has no BC subfield'.format(where, p))


def iter_blocks(path, start=0):
    """(file offset, block bytes) of every BGZF block from file offset `start` on.  ValueError on a cut or foreign block."""
    with open(path, 'rb') as f:
        f.seek(start)
        buf, base, p = b'', start, 0
        while True:
            if len(buf) - p < 18 or len(buf) - p < (_block_size(buf, p, path) or 1 << 30):
                more = f.read(_CHUNK)
                buf, base, p = buf[p:] + more, base + p, 0
                if not buf:
                    return
                if len(buf) < 18:
                    raise ValueError('{0}: truncated BGZF block at byte {1}'.format(path, base))
            total = _block_size(buf, p, path)
            if total is None or total > len(buf) - p:
                raise ValueError('{0}: truncated BGZF block at byte {1}'.format(path, base + p))
            yield base + p, memoryview(buf)[p:p + total]
            p += total


def bgzf_blocks(path):
    """Offsets, compressed sizes and inflated sizes of every block of a BGZF file (int64 arrays)."""
    offs, sizes, isizes = [], [], []
    for off, blk in iter_blocks(path):
        offs.append(off)
        sizes.append(len(blk))
        isizes.append(struct.unpack_from('<I', blk, len(blk) - 4)[0])
    return np.array(offs, np.int64), np.array(sizes, np.int64), np.array(isizes, np.int64)


def has_eof_block(path):
    """True when the file ends with BGZF's 28-byte empty block."""
    size = os.path.getsize(path)
    if size < len(BGZF_EOF):
        return False
    with open(path, 'rb') as f:
        f.seek(size - len(BGZF_EOF))
        return f.read() == BGZF_EOF


INFLATE_E_CRC = 8
INFLATE_ERRORS = {1: 'bad block type or header', 2: 'bad code lengths', 3: 'invalid code', 4: 'distance too far back',
                  5: 'input ended early', 6: 'inflated size differs from ISIZE', 7: 'bytes after the final deflate block',
                  8: 'CRC32 differs from the block trailer'}


class BgzfCrcError(ValueError):
    """A BGZF block that inflates to ISIZE bytes whose CRC32 is not the one in its trailer."""


def inflate_block(blk, verify=False):
    """
    The data of one BGZF block (raw deflate between the header and the CRC32 / ISIZE trailer).  verify: the data must have
    the trailer's CRC32 (BgzfCrcError, a ValueError).
    """
    xlen = struct.unpack_from('<H', blk, 10)[0]
    crc, isize = struct.unpack_from('<II', blk, len(blk) - 8)
    data = zlib.decompress(blk[12 + xlen:len(blk) - 8], -15)
    if len(data) != isize:
        raise ValueError('BGZF block inflates to {0} bytes, ISIZE says {1}'.format(len(data), isize))
    if verify and zlib.crc32(data) & 0xffffffff != crc:
        raise BgzfCrcError('BGZF block does not inflate: ' + INFLATE_ERRORS[INFLATE_E_CRC])
    return data


def _inflate_verified(blk):
    return inflate_block(blk, True)


def _block_error(path, offset, status):
    return '{0}: the BGZF block at byte {1} does not inflate: {2}'.format(path, offset, INFLATE_ERRORS.get(int(status), 'error {0}'.format(int(status))))


def block_crcs(blocks):
    """The CRC32 of the trailer of every block of a list of whole BGZF blocks (uint32; one entry for an empty list)."""
    crc = np.zeros(max(len(blocks), 1), np.uint32)
    for k, blk in enumerate(blocks):
        if len(blk) < 20:
            raise ValueError('BGZF block {0} is cut short ({1} bytes)'.format(k, len(blk)))
        crc[k] = struct.unpack_from('<I', blk, len(blk) - 8)[0]
    return crc


def _block_layout(blocks):
    """Blocks joined into one uint8 array, and per block the offset and length of its deflate payload and its ISIZE."""
    n = len(blocks)
    pay_off, pay_len, isize = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64)
    p = 0
    for k, blk in enumerate(blocks):
        if len(blk) < 20:
            raise ValueError('BGZF block {0} is cut short ({1} bytes)'.format(k, len(blk)))
        head = 12 + struct.unpack_from('<H', blk, 10)[0]
        if head + 8 > len(blk):
            raise ValueError('BGZF block {0} is cut short ({1} bytes)'.format(k, len(blk)))
        pay_off[k], pay_len[k], isize[k] = p + head, len(blk) - 8 - head, struct.unpack_from('<I', blk, len(blk) - 4)[0]
        p += len(blk)
    comp = np.frombuffer(b''.join(blocks), dtype=np.uint8) if p else np.zeros(1, np.uint8)
    return comp, p, pay_off, pay_len, isize


def inflate_blocks(blocks, device=None, verify=False):
    """
    The data of whole BGZF blocks (as iter_blocks yields them), inflated by the library's own DEFLATE decoder: on the host
    (device=None; no GPU needed) or on GPU `device`, one block per wavefront.  ValueError names the first block that does
    not decode or (verify) whose bytes do not have the CRC32 of its trailer.
    """
    blocks = list(blocks)
    n = len(blocks)
    comp, n_comp, pay_off, pay_len, isize = _block_layout(blocks)
    if n and int(isize[:n].max()) > 65536:
        raise ValueError('BGZF block {0} claims an inflated size of {1} bytes'.format(int(isize[:n].argmax()), int(isize[:n].max())))
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(isize[:n], out=out_off[1:])
    out = np.zeros(int(out_off[-1]) + 1, np.uint8)
    status = np.zeros(max(n, 1), np.int32)
    i64, i32, u8 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8
    args = (_ptr(comp, u8), n_comp, n, _ptr(pay_off, i64), _ptr(pay_len, i32), _ptr(out_off, i64), _ptr(out, u8), _ptr(status, i32))
    crc = _ptr(block_crcs(blocks), ctypes.c_uint32) if verify else None
    if device is None and not verify:
        _check(_lib.load().dn_bgzf_inflate_host(*args), 'dn_bgzf_inflate_host')
    elif device is None:
        _check(_lib.load().dn_bgzf_inflate_check_host(*(args + (crc,))), 'dn_bgzf_inflate_check_host')
    elif not verify:
        _check(_lib.load().dn_bgzf_inflate(int(device), *(args + (None, None))), 'dn_bgzf_inflate')
    else:
        _check(_lib.load().dn_bgzf_inflate_check(int(device), *(args + (None, None, crc))), 'dn_bgzf_inflate_check')
    _raise_status(status[:n], lambda k: 'BGZF block {0}'.format(k))
    data = out.tobytes()
    return [data[out_off[k]:out_off[k + 1]] for k in range(n)]


def _raise_status(status, where):
    bad = np.flatnonzero(status)
    if len(bad):
        k = int(bad[0])
        raise ValueError('{0} does not inflate: {1}'.format(where(k), INFLATE_ERRORS.get(int(status[k]), 'error {0}'.format(int(status[k])))))


def _raise_block_status(path, batch, status):
    """ValueError naming the file and the offset of the first of the (offset, block) pairs of batch whose status is not 0."""
    _raise_status(status[:len(batch)], lambda k: '{0}: the BGZF block at byte {1}'.format(path, batch[k][0]))


def _batched(blocks, window_bytes, size=0):
    """
    Lists of the (file offset, block) pairs that `blocks` yields: a list ends with the block that brings its inflated data to
    window_bytes.  size: what the first list counts before its first block (negative: bytes of that block that are not its).
    A loop over whole files drops its list (`del batch`) when it is done with it: otherwise the blocks of one window stay
    allocated while the next window's are read, which costs more than the marshalling of a window does.
    """
    batch = []
    for off, blk in blocks:
        batch.append((off, blk))
        size += struct.unpack_from('<I', blk, len(blk) - 4)[0]
        if size >= window_bytes:
            yield batch
            batch, size = [], 0
    if batch:
        yield batch


def _block_args(blocks):
    """
    What every inflate entry point of the library takes for whole BGZF blocks: the ctypes arguments (comp, n_comp, n_blocks,
    pay_off, pay_len), the blocks' ISIZEs as they are in the file (int64) and the status array the call fills.
    """
    comp, n_comp, pay_off, pay_len, isize = _block_layout(blocks)
    args = (_ptr(comp, ctypes.c_uint8), n_comp, len(blocks), _ptr(pay_off, ctypes.c_int64), _ptr(pay_len, ctypes.c_int32))
    return args, isize, np.zeros(max(len(blocks), 1), np.int32)


def _window_args(blocks, verify=False, expect_crc=None):
    """
    What the window entry points take: _block_args' arguments with the ISIZEs as their sixth, and the status array.  verify:
    the CRC32s of the blocks' trailers are announced first, through expect_crc (which takes the uint32 array).
    """
    args, isize, status = _block_args(blocks)
    if verify:
        expect_crc(block_crcs(blocks)[:len(blocks)])
    isize32 = np.where(isize > 2 ** 31 - 1, -1, isize).astype(np.int32)      # the library refuses a negative size
    return args + (_ptr(isize32, ctypes.c_int32),), status


def _zlib_inflate(path, batch, pool, verify=False):
    """
    The data of the blocks of batch, in file order, by zlib (in pool, when there is one).  verify: the first block whose data
    does not have the CRC32 of its trailer is a BgzfCrcError (a ValueError) naming the file and its offset.
    """
    blocks = [b for _, b in batch]
    one = _inflate_verified if verify else inflate_block
    data = []
    try:
        for d in (pool.map(one, blocks) if pool is not None else map(one, blocks)):      # in file order: the first bad block raises
            data.append(d)
    except BgzfCrcError:                                 # the blocks before it were good: this is the one, whatever its ISIZE
        raise BgzfCrcError(_block_error(path, batch[len(data)][0], INFLATE_E_CRC))
    return data


# --- header and index ----------------------------------------------------------------------------------------------------

def parse_header(data):
    """(header end, [(name, length)]) of inflated BAM bytes, or None while `data` holds less than the whole header."""
    if len(data) < 12:
        return None
    if bytes(data[:4]) != b'BAM\x01':
        raise ValueError('not a BAM file (magic {0!r})'.format(bytes(data[:4])))
    l_text = struct.unpack_from('<i', data, 4)[0]
    p = 8 + l_text
    if len(data) < p + 4:
        return None
    n_ref = struct.unpack_from('<i', data, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        if len(data) < p + 4:
            return None
        l_name = struct.unpack_from('<i', data, p)[0]
        if len(data) < p + 8 + l_name:
            return None
        name = bytes(data[p + 4:p + 4 + l_name]).rstrip(b'\x00').decode('ascii')
        refs.append((name, struct.unpack_from('<i', data, p + 4 + l_name)[0]))
        p += 8 + l_name
    return p, refs


def read_header(path, verify=False):
    """[(SQ name, length)] of a BAM file, in refID order.  verify: its blocks must have the CRC32s of their trailers."""
    data = bytearray()
    for off, blk in iter_blocks(path):
        try:
            data += inflate_block(blk, verify)
        except BgzfCrcError:
            raise ValueError(_block_error(path, off, INFLATE_E_CRC))
        got = parse_header(data)
        if got is not None:
            return got[1]
    raise ValueError('{0}: BAM header cut short'.format(path))


def read_bai(path):
    """
    A .bai index: (per reference a dict with `n_bin`, `pseudo` = (ref_beg, ref_end, n_mapped, n_unmapped) or None,
    `chunk_min` / `chunk_max` over all chunks of the real bins (None without any), n_no_coor or None).
    """
    with open(path, 'rb') as f:
        b = f.read()
    if b[:4] != b'BAI\x01':
        raise ValueError('{0} is not a .bai index'.format(path))
    n_ref = struct.unpack_from('<i', b, 4)[0]
    p, refs = 8, []
    try:
        for _ in range(n_ref):
            n_bin = struct.unpack_from('<i', b, p)[0]
            p += 4
            pseudo, lo, hi = None, None, None
            for _ in range(n_bin):
                bin_id, n_chunk = struct.unpack_from('<Ii', b, p)
                p += 8
                ch = np.frombuffer(b, dtype='<u8', count=2 * n_chunk, offset=p).reshape(n_chunk, 2)
                p += 16 * n_chunk
                if bin_id == PSEUDO_BIN:
                    pseudo = tuple(int(x) for x in ch.reshape(-1)[:4])
                elif n_chunk:
                    lo = int(ch[:, 0].min()) if lo is None else min(lo, int(ch[:, 0].min()))
                    hi = int(ch[:, 1].max()) if hi is None else max(hi, int(ch[:, 1].max()))
            n_intv = struct.unpack_from('<i', b, p)[0]
            p += 4 + 8 * n_intv
            refs.append({'n_bin': n_bin, 'pseudo': pseudo, 'chunk_min': lo, 'chunk_max': hi})
    except (struct.error, ValueError) as e:
        raise ValueError('{0}: truncated .bai index ({1})'.format(path, e))
    n_no_coor = struct.unpack_from('<Q', b, p)[0] if len(b) >= p + 8 else None
    return refs, n_no_coor


def reference_range(ref):
    """[begin, end) virtual offsets of one reference's records from its .bai entry, or None when it has no reads."""
    if ref['pseudo'] is not None:
        return ref['pseudo'][0], ref['pseudo'][1]
    if ref['chunk_min'] is None:
        return None
    return ref['chunk_min'], ref['chunk_max']


# --- framing and the device row store ------------------------------------------------------------------------------------

def frame_records(buf, tid=-1, last_pos=_INT32_MIN, device=None, segment_bytes=None, stats=None):
    """
    Start offsets (int64) of the complete records of inflated BAM bytes, the bytes they span (the rest is a record cut by
    the end of buf) and the last record's pos.  With tid >= 0 every record must belong to tid and be sorted (ValueError).
    Runs in the library's host code: no device needed.

    With `device` or `segment_bytes` the segmented algorithm of csrc/dn_frame.hip runs instead of the serial walk, with the
    same results and errors: on GPU `device`, or (device=None) its host build, which needs no GPU.  segment_bytes: at least
    64; None is the library's default.  stats, a dict, receives `segments`, `fixups` (segments whose guessed entry was not
    the true one and that were walked again) and `device_ms`.
    """
    a = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, np.uint8)
    cap = len(buf) // 36 + 1
    off = np.empty(cap, dtype=np.int64)
    n, used, lp = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(last_pos)
    lib = _lib.load()
    if device is None and segment_bytes is None:
        _check(lib.dn_bam_frame(_ptr(a, ctypes.c_uint8), len(buf), int(tid), ctypes.byref(lp), _ptr(off, ctypes.c_int64),
                                cap, ctypes.byref(n), ctypes.byref(used)), 'dn_bam_frame')
        if stats is not None:
            stats.update(segments=0, fixups=0, device_ms=0.0)
        return off[:n.value], int(used.value), int(lp.value)
    seg = 0 if segment_bytes is None else int(segment_bytes)
    if seg != 0 and seg < 64:
        raise ValueError('segment_bytes must be at least 64, not {0}'.format(segment_bytes))
    fix, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
    args = (_ptr(a, ctypes.c_uint8), len(buf), int(tid), ctypes.byref(lp), seg, _ptr(off, ctypes.c_int64), cap, ctypes.byref(n),
            ctypes.byref(used), ctypes.byref(fix))
    try:
        if device is None:
            _check(lib.dn_bam_frame_segments_host(*args), 'dn_bam_frame_segments_host')
        else:
            _check(lib.dn_bam_frame_device(int(device), *(args + (ctypes.byref(ms),))), 'dn_bam_frame_device')
    finally:
        if stats is not None:
            size = seg or int(lib.dn_bam_frame_segment_default())
            stats.update(segments=(len(buf) + size - 1) // size, fixups=int(fix.value), device_ms=float(ms.value))
    return off[:n.value], int(used.value), int(lp.value)


class DeviceRows(object):
    """The device-resident rows of one chromosome (dn_bam_rows): kept records in file order."""

    def __init__(self, tid, unique_alignment, paired, device=None):
        self.lib = _lib.load()
        self.paired = bool(paired)
        self.h = ctypes.c_void_p()
        dev = int(os.environ.get('LOCAL_RANK', 0)) if device is None else int(device)
        _check(self.lib.dn_bam_rows_create(dev, int(tid), 1 if unique_alignment else 0, 1 if paired else 0,
                                           ctypes.byref(self.h)), 'dn_bam_rows_create')

    def close(self):
        if self.h:
            self.lib.dn_bam_rows_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    def append(self, buf, rec_off):
        if len(rec_off) == 0:
            return
        a = np.frombuffer(buf, dtype=np.uint8)
        _check(self.lib.dn_bam_rows_append(self.h, _ptr(a, ctypes.c_uint8), len(buf), _ptr(rec_off, ctypes.c_int64),
                                           len(rec_off)), 'dn_bam_rows_append')

    def expect_crc(self, crc):
        """dn_bam_rows_expect_crc: the next inflate / inflate_framed checks its blocks against these CRC32s (one per block)."""
        crc = np.ascontiguousarray(crc, dtype=np.uint32)
        _check(self.lib.dn_bam_rows_expect_crc(self.h, _ptr(crc, ctypes.c_uint32) if len(crc) else None, len(crc)), 'dn_bam_rows_expect_crc')

    def inflate(self, carry, blocks, head_skip, tail_keep, verify=False):
        """
        dn_bam_rows_inflate: the next window (carry + the inflated blocks, trimmed) built on the device.  Returns a view of
        the library's host copy of it (valid until the next call), the status of every block and the kernel's ms.
        verify: every block, all of it, must have the CRC32 of its trailer (status 8 otherwise).
        """
        args, status = _window_args(blocks, verify, self.expect_crc)
        c = np.frombuffer(carry, dtype=np.uint8) if len(carry) else np.zeros(1, np.uint8)
        view, n_bytes, ms = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int64(0), ctypes.c_double(0.0)
        args = (_ptr(c, ctypes.c_uint8), len(carry)) + args + (int(head_skip), int(tail_keep), ctypes.byref(view), ctypes.byref(n_bytes),
                                                               _ptr(status, ctypes.c_int32), ctypes.byref(ms))
        _check(self.lib.dn_bam_rows_inflate(self.h, *args), 'dn_bam_rows_inflate')
        data = np.ctypeslib.as_array(view, shape=(n_bytes.value,)) if n_bytes.value else np.zeros(0, np.uint8)
        return data, status[:len(blocks)], float(ms.value)

    def frame_segment(self, segment_bytes):
        """The segment size of this store's device framing (None or 0: the library's default)."""
        _check(self.lib.dn_bam_rows_frame_segment(self.h, int(segment_bytes or 0)), 'dn_bam_rows_frame_segment')

    def append_framed(self, buf):
        """dn_bam_rows_append_framed: upload buf, frame it on the device, decode and append.  Returns the bytes consumed."""
        a = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, np.uint8)
        used = ctypes.c_int64(0)
        _check(self.lib.dn_bam_rows_append_framed(self.h, _ptr(a, ctypes.c_uint8), len(buf), ctypes.byref(used)), 'dn_bam_rows_append_framed')
        return int(used.value)

    def inflate_framed(self, blocks, head_skip, tail_keep, verify=False):
        """
        dn_bam_rows_inflate_framed: the next window inflated, framed, decoded and appended on the device; the record its end
        cuts stays there.  Returns the status of every block, the bytes carried over, and the ms of inflate and framing.
        verify: as for inflate.
        """
        args, status = _window_args(blocks, verify, self.expect_crc)
        n_bytes, n_carry, ms, fms = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        args += (int(head_skip), int(tail_keep), _ptr(status, ctypes.c_int32), ctypes.byref(n_bytes), ctypes.byref(n_carry), ctypes.byref(ms),
                 ctypes.byref(fms))
        _check(self.lib.dn_bam_rows_inflate_framed(self.h, *args), 'dn_bam_rows_inflate_framed')
        return status[:len(blocks)], int(n_carry.value), float(ms.value), float(fms.value)

    def frame_info(self):
        """(segments, fix-ups, framing's device ms, decode's host ms) summed over the windows this store framed on the device."""
        n_seg, n_fix, ms, dms = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        _check(self.lib.dn_bam_rows_frame_info(self.h, ctypes.byref(n_seg), ctypes.byref(n_fix), ctypes.byref(ms), ctypes.byref(dms)),
               'dn_bam_rows_frame_info')
        return int(n_seg.value), int(n_fix.value), float(ms.value), float(dms.value)

    def append_resident(self, rec_off):
        if len(rec_off) == 0:
            return
        _check(self.lib.dn_bam_rows_append_resident(self.h, _ptr(rec_off, ctypes.c_int64), len(rec_off)), 'dn_bam_rows_append_resident')

    def info(self):
        n, n_ops, n_names, mk = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        _check(self.lib.dn_bam_rows_info(self.h, ctypes.byref(n), ctypes.byref(n_ops), ctypes.byref(n_names), ctypes.byref(mk)),
               'dn_bam_rows_info')
        return n.value, n_ops.value, n_names.value, mk.value

    def keys(self):
        """qname_unpaired of every row as a fixed-width bytes array (numpy S)."""
        n, _, _, mk = self.info()
        width = max(mk, 1)
        out = np.zeros((max(n, 1), width), dtype=np.uint8)
        _check(self.lib.dn_bam_rows_keys(self.h, width, _ptr(out, ctypes.c_uint8)), 'dn_bam_rows_keys')
        return out[:n].view('S{0}'.format(width)).reshape(n)

    def fetch(self):
        """(pos int64, op_beg int64, n_op int32, ops uint32, name_beg int64, name_len int32, names uint8) of the rows."""
        n, n_ops, n_names, _ = self.info()
        pos, op_beg, name_beg = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        n_op, name_len = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        ops, names = np.zeros(max(n_ops, 1), np.uint32), np.zeros(max(n_names, 1), np.uint8)
        i64, i32 = ctypes.c_int64, ctypes.c_int32
        _check(self.lib.dn_bam_rows_fetch(self.h, _ptr(pos, i64), _ptr(op_beg, i64), _ptr(n_op, i32), _ptr(ops, ctypes.c_uint32),
                                          _ptr(name_beg, i64), _ptr(name_len, i32), _ptr(names, ctypes.c_uint8)), 'dn_bam_rows_fetch')
        return pos[:n], op_beg[:n], n_op[:n], ops[:n_ops], name_beg[:n], name_len[:n], names[:n_names]

    def pair(self, fetch=False):
        """
        dn_bam_rows_pair: pair the mates on the device and keep the result there.  Rows go in ascending qname_unpaired order,
        equal keys in file order: np.argsort(self.keys(), kind='stable').  Returns (order int32, pair_id int32, number of ids,
        device ms) with fetch=True, (None, None, number of ids, device ms) otherwise.
        """
        n = self.info()[0] if fetch else 0
        order = np.zeros(max(n, 1), np.int32) if fetch else None
        pair_id = np.zeros(max(n, 1), np.int32) if fetch else None
        n_ids, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _check(self.lib.dn_bam_rows_pair(self.h, _ptr(order, ctypes.c_int32), _ptr(pair_id, ctypes.c_int32), ctypes.byref(n_ids),
                                         ctypes.byref(ms)), 'dn_bam_rows_pair')
        if fetch:
            return order[:n], pair_id[:n], int(n_ids.value), float(ms.value)
        return None, None, int(n_ids.value), float(ms.value)

    def coverage(self, ann, pair='host'):
        """
        dn_bam_rows_coverage: the outputs of reads.device_read_coverage for the stored rows.  A paired store's mates are
        paired on the host in the reference's order (pair_order; pair='host') or on the device with equal keys in file order
        (self.pair(); pair='device'), which moves no keys to the host; self.pair_ms is then the pairing's device ms.
        """
        if pair not in ('host', 'device'):
            raise ValueError("pair must be 'host' or 'device', not {0!r}".format(pair))
        order, pair_id, n_ids = None, None, 0
        self.pair_ms = 0.0
        if self.paired and pair == 'device':
            self.pair_ms = self.pair()[3]
        elif self.paired:
            order, pair_id, n_ids = pair_order(self.keys())
        i32, i64, dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
        n_genes = len(ann.genes)
        counts = np.zeros(max(n_genes, 1), dtype=np.int64)
        ol_cov = np.zeros(max(int(ann.ol_cov_off[-1]), 1), dtype=np.int64)
        cap = max(ann.exon_union_len, 1)
        csr_idx = np.zeros(cap, dtype=np.int32)
        csr_val = np.zeros(cap, dtype=np.int64)
        nnz, n_iso_reads, ms = ctypes.c_int64(0), ctypes.c_int64(0), dbl(0.0)
        rc = self.lib.dn_bam_rows_coverage(self.h, _ptr(order, i32), _ptr(pair_id, i32), int(n_ids),
                                           ann.chrom_len, ann.keep_lo, ann.keep_hi,
                                           len(ann.exon_iv), _ptr(ann.exon_iv, i64),
                                           len(ann.group_iv), _ptr(ann.group_iv, i64), _ptr(ann.group_gene_off, i32),
                                           _ptr(ann.ol_gene, i32), _ptr(ann.ol_gs0, i64), _ptr(ann.ol_cov_off, i64),
                                           _ptr(ann.ol_exon_off, i32), _ptr(ann.ol_exon, i64),
                                           len(ann.iso_iv), _ptr(ann.iso_iv, i64), _ptr(ann.iso_gene, i32),
                                           len(ann.iso_union), _ptr(ann.iso_union, i64),
                                           n_genes, _ptr(counts, i64), _ptr(ol_cov, i64), cap, ctypes.byref(nnz),
                                           _ptr(csr_idx, i32), _ptr(csr_val, i64), ctypes.byref(n_iso_reads), ctypes.byref(ms))
        _check(rc, 'dn_bam_rows_coverage')
        k = int(nnz.value)
        return counts[:n_genes], ol_cov, csr_idx[:k].copy(), csr_val[:k].copy(), int(n_iso_reads.value), float(ms.value)


def pair_order(keys):
    """
    The row order of DataFrame.sort_values('qname_unpaired') (pandas' default quicksort) on rows in file order with these
    keys, and the pair id of each row taken in that order: (order int32, pair_id int32, number of ids).
    """
    keys = np.asarray(keys)
    order = np.argsort(keys, kind='quicksort').astype(np.int32)
    sk = keys[order]
    pair_id = np.zeros(len(sk), dtype=np.int32)
    if len(sk) > 1:
        np.cumsum(sk[1:] != sk[:-1], out=pair_id[1:])
    return order, pair_id, int(pair_id[-1]) + 1 if len(sk) else 0


def pair_rows(keys):
    """
    The order and pair ids of DeviceRows.pair() for these keys (an S-dtype array, or a list of bytes), computed by the
    library's host build of the same passes (dn_bam_pair_host; no device needed): (order int32, pair_id int32, number of
    ids) with order == np.argsort(keys, kind='stable').
    """
    keys = [bytes(k) for k in (keys.tolist() if isinstance(keys, np.ndarray) else keys)]
    n = len(keys)
    key_len = np.array([len(k) for k in keys], dtype=np.int32).reshape(n)
    name_beg = np.zeros(max(n, 1), dtype=np.int64)
    if n > 1:
        np.cumsum(key_len[:-1], out=name_beg[1:n])
    blob = b''.join(keys)
    names = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)
    order, pair_id = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    n_ids = ctypes.c_int64(0)
    key_len = key_len if n else np.zeros(1, np.int32)
    _check(_lib.load().dn_bam_pair_host(n, _ptr(name_beg, ctypes.c_int64), _ptr(key_len, ctypes.c_int32), _ptr(names, ctypes.c_uint8),
                                        _ptr(order, ctypes.c_int32), _ptr(pair_id, ctypes.c_int32), ctypes.byref(n_ids)), 'dn_bam_pair_host')
    return order[:n], pair_id[:n], int(n_ids.value)


def cigar_strings(op_beg, n_op, ops):
    """pysam's cigarstring of every row (None for a row without ops)."""
    lens, codes = (ops >> 4).tolist(), (ops & 15).tolist()
    tok = [str(l) + CIGAR_OPS[c] if c < 9 else str(l) + '?' for l, c in zip(lens, codes)]
    return [''.join(tok[b:b + k]) if k else None for b, k in zip(op_beg.tolist(), n_op.tolist())]


# --- the processor -------------------------------------------------------------------------------------------------------

class NativeBamReadsProcessor(BamReadsProcessor):

    def __init__(self, bam_file, index_file, chroms=None, n_jobs=1, output_dir=None, unique_alignment=True, verbose=True,
                 window_bytes=256 << 20, inflate='host', frame='host', frame_segment_bytes=None, verify=False, pair='host'):
        """
        BamReadsProcessor on the library's own BAM reader: no pysam.  n_jobs sizes the thread pool that inflates BGZF
        blocks; window_bytes bounds the inflated bytes held (on the host and on the device) besides the chromosome's rows.
        inflate='host' inflates with zlib in that pool; inflate='device' hands the compressed blocks to the library's DEFLATE
        kernel (device_rows, and with it coverage and load_chromosome_reads; the header and the strand check stay on zlib).
        frame='host' finds the record starts of a window with the library's serial host walk; frame='device' finds them on
        the GPU (with either inflate; the strand check stays on the host walk), in segments of frame_segment_bytes (None:
        the library's default).  timing then has frame_device_ms and frame_fixups instead of frame_s.
        verify=True compares every block that is inflated -- by either side, and also for the header and the strand check
        -- with the CRC32 of its trailer; a block that differs is a ValueError naming the file and the block's offset.
        pair='host' pairs the mates of a paired-end file on the host, in the reference's order (pair_order); pair='device'
        pairs them on the GPU, equal keys in file order (DeviceRows.pair), with either inflate and frame; timing then has
        pair_device_ms.  Coverage can differ between the two only where a pair's mates overlap on the reference.  No effect on
        a single-end file, nor on load_chromosome_reads.
        """
        if inflate not in ('host', 'device'):
            raise ValueError("inflate must be 'host' or 'device', not {0!r}".format(inflate))
        if frame not in ('host', 'device'):
            raise ValueError("frame must be 'host' or 'device', not {0!r}".format(frame))
        if pair not in ('host', 'device'):
            raise ValueError("pair must be 'host' or 'device', not {0!r}".format(pair))
        self.inflate = inflate
        self.frame = frame
        self.pair = pair
        self.frame_segment_bytes = frame_segment_bytes
        self.verify = bool(verify)
        self.window_bytes = max(int(window_bytes), 1)
        self.timing = {}
        super(NativeBamReadsProcessor, self).__init__(bam_file, index_file, chroms=chroms, n_jobs=n_jobs, output_dir=output_dir,
                                                      unique_alignment=unique_alignment, verbose=verbose)

    def _open_backend(self):
        self._refs = None
        self._index = None

    def _load(self):
        if self._refs is None:
            if not has_eof_block(self.filename):
                raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(self.filename))
            self._refs = read_header(self.filename, self.verify)
            self._index, _ = read_bai(self.index_filename)
            if len(self._index) != len(self._refs):
                raise ValueError('{0} indexes {1} references, {2} has {3}'.format(
                    self.index_filename, len(self._index), self.filename, len(self._refs)))
            self._tid = {name: k for k, (name, _) in enumerate(self._refs)}

    def _reference_lengths(self):
        self._load()
        return {name: length for name, length in self._refs}

    def _batches(self, chrom, window_bytes=None):
        """((file offset, block) of about window_bytes of inflated data, cbeg, ubeg, cend, uend) over chrom's index range."""
        self._load()
        rng = reference_range(self._index[self._tid[chrom]])
        if rng is None:
            return
        window_bytes = window_bytes or self.window_bytes
        vbeg, vend = rng
        cbeg, ubeg, cend, uend = vbeg >> 16, vbeg & 0xffff, vend >> 16, vend & 0xffff
        in_range = itertools.takewhile(lambda ob: ob[0] < cend or (ob[0] == cend and uend > 0), iter_blocks(self.filename, cbeg))
        for batch in _batched(in_range, window_bytes):
            yield batch, cbeg, ubeg, cend, uend

    def windows(self, chrom, window_bytes=None):
        """
        Inflated bytes of the blocks that hold chrom's records, about window_bytes at a time; a record may be cut at the
        end of one window and continue in the next.  Adds host inflate seconds to self.timing['inflate_s'].
        """
        pool = ThreadPoolExecutor(max_workers=int(self.n_jobs)) if int(self.n_jobs) > 1 else None
        try:
            for batch, cbeg, ubeg, cend, uend in self._batches(chrom, window_bytes):
                yield self._inflate(batch, pool, cbeg, ubeg, cend, uend)
        finally:
            if pool is not None:
                pool.shutdown()

    def _inflate(self, batch, pool, cbeg, ubeg, cend, uend):
        t0 = time.perf_counter()
        data = _zlib_inflate(self.filename, batch, pool, self.verify)
        for k, (off, _) in enumerate(batch):
            if off == cend:
                data[k] = data[k][:uend]
            if off == cbeg:
                data[k] = data[k][ubeg:]
        out = b''.join(data)
        self.timing['inflate_s'] = self.timing.get('inflate_s', 0.0) + time.perf_counter() - t0
        return out

    def _leading_query_names(self, chrom):
        self._load()
        names, carry, last = [], b'', _INT32_MIN
        for win in self.windows(chrom, window_bytes=1 << 20):
            data = carry + win
            off, used, last = frame_records(data, self._tid[chrom], last)
            for o in off.tolist():
                l_name = data[o + 12]
                names.append(data[o + 36:o + 35 + l_name].decode('ascii', 'replace'))
                if len(names) > 300:
                    return names
            carry = data[used:]
        return names

    def device_rows(self, chrom, device=None):
        """The chromosome's kept records as a DeviceRows store (file order)."""
        self._load()
        rows = DeviceRows(self._tid[chrom], self.unique_alignment, self.paired, device)
        carry, last = b'', _INT32_MIN
        t = self.timing
        try:
            if self.frame == 'device':
                return self._device_framed(chrom, rows)
            if self.inflate == 'device':
                return self._device_windows(chrom, rows)
            for win in self.windows(chrom):
                data = carry + win if carry else win
                t0 = time.perf_counter()
                off, used, last = frame_records(data, self._tid[chrom], last)
                t1 = time.perf_counter()
                rows.append(data, off)
                t2 = time.perf_counter()
                t['frame_s'] = t.get('frame_s', 0.0) + t1 - t0
                t['decode_s'] = t.get('decode_s', 0.0) + t2 - t1
                carry = data[used:]
            if carry:
                raise ValueError('{0}: a record of {1} is cut short at the end of its index range'.format(self.filename, chrom))
        except Exception:
            rows.close()
            raise
        return rows

    def _device_windows(self, chrom, rows):
        """device_rows with inflate='device': every window is inflated into the row store and decoded where it lies."""
        carry, last = b'', _INT32_MIN
        t = self.timing
        for batch, cbeg, ubeg, cend, uend in self._batches(chrom):
            t0 = time.perf_counter()
            data, status, ms = rows.inflate(carry, [b for _, b in batch], ubeg if batch[0][0] == cbeg else 0,
                                            uend if batch[-1][0] == cend else -1, self.verify)
            t1 = time.perf_counter()
            _raise_block_status(self.filename, batch, status)
            off, used, last = frame_records(data, self._tid[chrom], last)
            t2 = time.perf_counter()
            rows.append_resident(off)
            t3 = time.perf_counter()
            t['inflate_s'] = t.get('inflate_s', 0.0) + t1 - t0
            t['inflate_device_ms'] = t.get('inflate_device_ms', 0.0) + ms
            t['frame_s'] = t.get('frame_s', 0.0) + t2 - t1
            t['decode_s'] = t.get('decode_s', 0.0) + t3 - t2
            carry = data[used:].tobytes()
        if carry:
            raise ValueError('{0}: a record of {1} is cut short at the end of its index range'.format(self.filename, chrom))
        return rows

    def _device_framed(self, chrom, rows):
        """device_rows with frame='device': every window is framed on the device, wherever it was inflated."""
        t = self.timing
        cut = '{0}: a record of {1} is cut short at the end of its index range'.format(self.filename, chrom)
        rows.frame_segment(self.frame_segment_bytes)
        calls = 0.0                         # seconds in the library's one call per window: it splits them (frame_info)
        try:
            if self.inflate == 'device':
                n_carry = 0
                for batch, cbeg, ubeg, cend, uend in self._batches(chrom):
                    t0 = time.perf_counter()
                    status, n_carry, ms, fms = rows.inflate_framed([b for _, b in batch], ubeg if batch[0][0] == cbeg else 0,
                                                                   uend if batch[-1][0] == cend else -1, self.verify)
                    t1 = time.perf_counter()
                    _raise_block_status(self.filename, batch, status)
                    t['inflate_device_ms'] = t.get('inflate_device_ms', 0.0) + ms
                    calls += t1 - t0
                if n_carry:
                    raise ValueError(cut)
            else:
                carry = b''
                for win in self.windows(chrom):
                    data = carry + win if carry else win
                    t0 = time.perf_counter()
                    used = rows.append_framed(data)
                    calls += time.perf_counter() - t0
                    carry = data[used:]
                if carry:
                    raise ValueError(cut)
        finally:
            _, fixups, ms, decode_ms = rows.frame_info()
            t['frame_device_ms'] = t.get('frame_device_ms', 0.0) + ms
            t['frame_fixups'] = t.get('frame_fixups', 0) + fixups
            t['decode_s'] = t.get('decode_s', 0.0) + 1e-3 * decode_ms
            # what is left of the calls: the copy of the window (inflate='host') or of its blocks and their inflate ('device')
            rest = max(calls - 1e-3 * (ms + decode_ms), 0.0)
            key = 'inflate_s' if self.inflate == 'device' else 'upload_s'
            t[key] = t.get(key, 0.0) + rest
        return rows

    def load_chromosome_reads(self, chrom):
        """
        The reference's DataFrame of one chromosome's reads (`qname`, `pos`, `cigar`, plus `qname_unpaired` and sorted by
        it when paired), built from the device-decoded rows.
        """
        rows = self.device_rows(chrom)
        try:
            pos, op_beg, n_op, ops, name_beg, name_len, names = rows.fetch()
        finally:
            rows.close()
        nb = names.tobytes()
        qname = [nb[b:b + k].decode('ascii', 'replace') for b, k in zip(name_beg.tolist(), name_len.tolist())]
        return reads_frame(list(zip(qname, pos.tolist(), cigar_strings(op_beg, n_op, ops))), self.paired)

    def _chromosome_coverage(self, chrom, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df):
        ann = Annotation(chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df)
        rows = self.device_rows(chrom)
        try:
            n_reads = rows.info()[0]
            t0 = time.perf_counter()
            counts, ol_cov, idx, val, n_iso_reads, ms = rows.coverage(ann, self.pair)
            self.timing['coverage_s'] = self.timing.get('coverage_s', 0.0) + time.perf_counter() - t0
            self.timing['coverage_device_ms'] = self.timing.get('coverage_device_ms', 0.0) + ms
            if self.pair == 'device':
                self.timing['pair_device_ms'] = self.timing.get('pair_device_ms', 0.0) + rows.pair_ms
        finally:
            rows.close()
        csr, ol_cov_dict, read_counts = coverage_outputs(ann, counts, ol_cov, idx, val, n_iso_reads)
        return csr, ol_cov_dict, read_counts, n_reads


# --- creating an index ---------------------------------------------------------------------------------------------------

class BamIndex(object):
    """
    A .bai index.  `refs` holds per reference a dict with `bins`, the list of (bin id, chunks) in the order of the file --
    chunks a (n, 2) uint64 array of [begin, end) virtual offsets; the pseudo-bin 37450 is one of the entries -- and
    `ioffset`, the linear index (uint64).  build_index writes the bins in ascending order and the pseudo-bin last;
    parse_bai keeps whatever order the file has, so tobytes() gives the file back.  n_no_coor: the count of records
    without a reference, None for a file that ends before it.
    """

    def __init__(self, refs, n_no_coor=None):
        self.refs = refs
        self.n_no_coor = n_no_coor

    def pseudo(self, tid):
        """(offset of the first record, end of the last, mapped, unmapped) of a reference, or None without a pseudo-bin."""
        for bin_id, ch in self.refs[tid]['bins']:
            if bin_id == PSEUDO_BIN:
                return tuple(int(x) for x in ch.reshape(-1)[:4])
        return None

    def tobytes(self):
        out = [b'BAI\x01', struct.pack('<i', len(self.refs))]
        for ref in self.refs:
            out.append(struct.pack('<i', len(ref['bins'])))
            for bin_id, ch in ref['bins']:
                out.append(struct.pack('<Ii', bin_id, len(ch)))
                out.append(np.ascontiguousarray(ch, dtype='<u8').tobytes())
            out.append(struct.pack('<i', len(ref['ioffset'])))
            out.append(np.ascontiguousarray(ref['ioffset'], dtype='<u8').tobytes())
        if self.n_no_coor is not None:
            out.append(struct.pack('<Q', self.n_no_coor))
        return b''.join(out)


def parse_bai(path):
    """The whole of a .bai index file as a BamIndex."""
    with open(path, 'rb') as f:
        b = f.read()
    if b[:4] != b'BAI\x01':
        raise ValueError('{0} is not a .bai index'.format(path))
    try:
        n_ref = struct.unpack_from('<i', b, 4)[0]
        p, refs = 8, []
        for _ in range(n_ref):
            n_bin = struct.unpack_from('<i', b, p)[0]
            p += 4
            bins = []
            for _ in range(n_bin):
                bin_id, n_chunk = struct.unpack_from('<Ii', b, p)
                p += 8
                bins.append((bin_id, np.frombuffer(b, dtype='<u8', count=2 * n_chunk, offset=p).reshape(n_chunk, 2).astype(np.uint64)))
                p += 16 * n_chunk
            n_intv = struct.unpack_from('<i', b, p)[0]
            p += 4
            refs.append({'bins': bins, 'ioffset': np.frombuffer(b, dtype='<u8', count=n_intv, offset=p).astype(np.uint64)})
            p += 8 * n_intv
    except (struct.error, ValueError) as e:
        raise ValueError('{0}: truncated .bai index ({1})'.format(path, e))
    return BamIndex(refs, struct.unpack_from('<Q', b, p)[0] if len(b) >= p + 8 else None)


def write_bai(index, path):
    """Write a BamIndex to `path`: to a temporary file next to it, renamed when complete."""
    tmp = '{0}.tmp{1}'.format(path, os.getpid())
    try:
        with open(tmp, 'wb') as f:
            f.write(index.tobytes())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def _host_inflate(bam_file, batch, pool, verify=False):
    """
    The data of the blocks of batch by zlib (verify: and their CRC32s by zlib.crc32, in the same pool); a block that fails
    is named with the text of the library's own decoder.
    """
    try:
        return _zlib_inflate(bam_file, batch, pool, verify)
    except BgzfCrcError:                                 # a wrong CRC32: _zlib_inflate has named the block
        raise
    except (zlib.error, ValueError, struct.error) as e:
        blocks = [b for _, b in batch]
        args, isize, status = _block_args(blocks)
        n = len(blocks)
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum(np.clip(isize[:n], 0, 65536), out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 1, np.uint8)
        if n and int(isize[:n].max()) <= 65536:
            crc = _ptr(block_crcs(blocks), ctypes.c_uint32) if verify else None
            args += (_ptr(out_off, ctypes.c_int64), _ptr(out, ctypes.c_uint8), _ptr(status, ctypes.c_int32), crc)
            _check(_lib.load().dn_bgzf_inflate_check_host(*args), 'dn_bgzf_inflate_check_host')
            _raise_block_status(bam_file, batch, status)
        raise ValueError('{0}: a BGZF block at or after byte {1} does not inflate: {2}'.format(bam_file, batch[0][0], e))


def build_index(bam_file, device=None, n_jobs=1, window_bytes=256 << 20, segment_bytes=None, stats=None, verify=False):
    """
    The .bai index of a coordinate-sorted BAM file as a BamIndex, from one pass over all its records (csrc/dn_bai.hip; the
    index is defined in include/degnorm_amd.h).  device=k: the blocks of about window_bytes of inflated data go to GPU k as
    they are in the file and are inflated, framed and indexed there; only the tables of run heads and linear-index claims
    come back.  device=None: the blocks are inflated with zlib in n_jobs threads and the library's host build of the same
    source walks them; no GPU is needed.  Both give the same index and the same errors (ValueError naming the file and
    the record).  verify: every block must have the CRC32 of its trailer, checked where the block is inflated (ValueError
    naming the file and the block's offset).  segment_bytes: of the framing (None: the library's default).  stats, a dict, receives
    `inflate_device_ms`, `frame_device_ms`, `index_device_ms`, `frame_fixups`, `records`, `chunks` and `windows`.
    """
    if not has_eof_block(bam_file):
        raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(bam_file))
    if segment_bytes is not None and int(segment_bytes) < 64:
        raise ValueError('segment_bytes must be at least 64, not {0}'.format(segment_bytes))
    window_bytes = max(int(256 << 20 if window_bytes is None else window_bytes), 1)
    lib = _lib.load()
    i64, i32, u8, u64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8, ctypes.c_uint64
    pool = ThreadPoolExecutor(max_workers=int(n_jobs)) if device is None and int(n_jobs) > 1 else None
    h = ctypes.c_void_p()
    ms = {'inflate_device_ms': 0.0, 'frame_device_ms': 0.0, 'index_device_ms': 0.0}
    end = {'coffset': None, 'open': False}          # the block behind the last one that holds a byte

    def blocks():
        for off, blk in iter_blocks(bam_file):
            if end['open']:
                end['coffset'] = off
            end['open'] = struct.unpack_from('<I', blk, len(blk) - 4)[0] > 0
            yield off, blk

    def call(rc, what):
        try:
            _check(rc, what)
        except ValueError as e:
            raise ValueError('{0}: {1}'.format(bam_file, e))

    def window(batch, head_skip):
        n_rec = i64(0)
        coffset = np.array([off for off, _ in batch], dtype=np.int64)
        if device is None:
            data = _host_inflate(bam_file, batch, pool, verify)
            isize = np.array([len(d) for d in data], dtype=np.int64)
            isize32 = np.where(isize > 2 ** 31 - 1, -1, isize).astype(np.int32)
            joined = np.frombuffer(b''.join(data), dtype=np.uint8) if int(isize.sum()) else np.zeros(1, np.uint8)
            call(lib.dn_bai_window_host(h, _ptr(joined, u8), int(isize.sum()), len(batch), _ptr(isize32, i32), _ptr(coffset, i64),
                                        int(head_skip), ctypes.byref(n_rec)), 'dn_bai_window_host')
            return
        args, status = _window_args([b for _, b in batch], verify, lambda crc: call(
            lib.dn_bai_expect_crc(h, _ptr(crc, ctypes.c_uint32), len(crc)), 'dn_bai_expect_crc'))
        t = [ctypes.c_double(0.0) for _ in range(3)]
        args += (_ptr(coffset, i64), int(head_skip), _ptr(status, i32), ctypes.byref(n_rec), ctypes.byref(t[0]), ctypes.byref(t[1]),
                 ctypes.byref(t[2]))
        call(lib.dn_bai_window(h, *args), 'dn_bai_window')
        for key, v in zip(('inflate_device_ms', 'frame_device_ms', 'index_device_ms'), t):
            ms[key] += float(v.value)
        _raise_block_status(bam_file, batch, status)

    try:
        # the header, on zlib whatever the device: it may span several blocks
        _, head_blocks, _, head_skip, refs = _header_data(bam_file, verify)
        call(lib.dn_bai_create(-1 if device is None else int(device), len(refs), int(segment_bytes or 0), ctypes.byref(h)), 'dn_bai_create')
        # the first window starts inside the block in which the header ends, and holds the bytes behind the header
        for batch in _batched(itertools.islice(blocks(), head_blocks - 1, None), window_bytes, -head_skip):
            window(batch, head_skip)
            head_skip = 0
            del batch
        if end['coffset'] is None or end['open']:
            raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(bam_file))
        sizes = np.zeros(8, dtype=np.int64)
        call(lib.dn_bai_finish(h, int(end['coffset']) << 16, _ptr(sizes, i64)), 'dn_bai_finish')
        n_bins, n_chunks, n_intv = (int(x) for x in sizes[:3])
        n_ref = len(refs)
        ref_n_bin, ref_n_intv = np.zeros(max(n_ref, 1), np.int32), np.zeros(max(n_ref, 1), np.int32)
        pseudo = np.zeros(max(4 * n_ref, 1), np.uint64)
        bin_id, bin_n_chunk = np.zeros(max(n_bins, 1), np.int32), np.zeros(max(n_bins, 1), np.int32)
        chunks, ioffset = np.zeros(max(2 * n_chunks, 1), np.uint64), np.zeros(max(n_intv, 1), np.uint64)
        call(lib.dn_bai_fetch(h, _ptr(ref_n_bin, i32), _ptr(ref_n_intv, i32), _ptr(pseudo, u64), _ptr(bin_id, i32), _ptr(bin_n_chunk, i32),
                              _ptr(chunks, u64), _ptr(ioffset, u64)), 'dn_bai_fetch')
    finally:
        if h:
            lib.dn_bai_destroy(h)
        if pool is not None:
            pool.shutdown()
    out, b, c, w = [], 0, 0, 0
    chunks = chunks[:2 * n_chunks].reshape(n_chunks, 2)
    for r in range(n_ref):
        bins = []
        for k in range(b, b + int(ref_n_bin[r])):
            bins.append((int(bin_id[k]), chunks[c:c + int(bin_n_chunk[k])].copy()))
            c += int(bin_n_chunk[k])
        b += int(ref_n_bin[r])
        if bins:
            bins.append((PSEUDO_BIN, pseudo[4 * r:4 * r + 4].reshape(2, 2).copy()))
        out.append({'bins': bins, 'ioffset': ioffset[w:w + int(ref_n_intv[r])].copy()})
        w += int(ref_n_intv[r])
    if stats is not None:
        stats.update(ms, frame_fixups=int(sizes[6]), records=int(sizes[3]), chunks=n_chunks, windows=int(sizes[5]))
    return BamIndex(out, int(sizes[4]))


def create_index(bam_file, bai_file=None, overwrite=False, **kw):
    """Build the index of bam_file (build_index's keywords) and write it to bai_file (default bam_file + '.bai'); its path."""
    bai_file = bam_file + '.bai' if bai_file is None else bai_file
    if os.path.exists(bai_file) and not overwrite:
        raise FileExistsError('{0} exists; pass overwrite=True to replace it'.format(bai_file))
    return write_bai(build_index(bam_file, **kw), bai_file)


def verify_bgzf(path, device=None, n_jobs=1, window_bytes=256 << 20):
    """
    Check a whole BGZF file as `bgzip -t` does: it ends with the end-of-file block, and every block inflates to its ISIZE
    bytes, which have the CRC32 of its trailer.  device=k: the blocks of about window_bytes of inflated data go to GPU k as
    they are in the file, every wavefront inflates and checks one, and only the statuses come back -- no inflated byte is
    written or copied.  device=None: zlib and zlib.crc32 in n_jobs threads.  ValueError names the file and the first bad
    block.  Returns {'blocks', 'compressed_bytes', 'inflated_bytes', 'device_ms'}.
    """
    if not has_eof_block(path):
        raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(path))
    window_bytes = max(int(256 << 20 if window_bytes is None else window_bytes), 1)
    out = {'blocks': 0, 'compressed_bytes': 0, 'inflated_bytes': 0, 'device_ms': 0.0}
    pool = ThreadPoolExecutor(max_workers=int(n_jobs)) if device is None and int(n_jobs) > 1 else None
    i64, i32 = ctypes.c_int64, ctypes.c_int32

    def window(batch):
        blocks = [b for _, b in batch]
        if device is None:
            _host_inflate(path, batch, pool, True)
            return
        args, isize, status = _block_args(blocks)
        n = len(blocks)
        if int(isize[:n].max()) > 65536:
            k = int(isize[:n].argmax())
            raise ValueError('{0}: the BGZF block at byte {1} claims an inflated size of {2} bytes'.format(path, batch[k][0], int(isize[k])))
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum(isize[:n], out=out_off[1:])
        ms = ctypes.c_double(0.0)
        args += (_ptr(out_off, i64), None, _ptr(status, i32), None, ctypes.byref(ms), _ptr(block_crcs(blocks), ctypes.c_uint32))
        _check(_lib.load().dn_bgzf_inflate_check(int(device), *args), 'dn_bgzf_inflate_check')
        out['device_ms'] += float(ms.value)
        _raise_block_status(path, batch, status)

    try:
        for batch in _batched(iter_blocks(path), window_bytes):
            out['blocks'] += len(batch)
            out['compressed_bytes'] += sum(len(blk) for _, blk in batch)
            out['inflated_bytes'] += sum(struct.unpack_from('<I', blk, len(blk) - 4)[0] for _, blk in batch)
            window(batch)
            del batch
    finally:
        if pool is not None:
            pool.shutdown()
    return out


def reg2bins(beg, end):
    """The bins that may hold records overlapping [beg, end) (SAM specification 5.3)."""
    beg, end = max(int(beg), 0), min(int(end), 1 << 29) - 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def index_chunks(index, tid, beg, end):
    """
    The [begin, end) virtual-offset ranges a reader has to scan for the records of reference tid that overlap [beg, end):
    the chunks of reg2bins(beg, end) that end above the linear index's lower bound for beg, sorted and coalesced.
    """
    ref = index.refs[tid]
    ioffset = ref['ioffset']
    low = int(ioffset[min(max(int(beg), 0) >> 14, len(ioffset) - 1)]) if len(ioffset) else 0
    want = set(reg2bins(beg, end))
    found = sorted((int(b), int(e)) for bin_id, ch in ref['bins'] if bin_id in want for b, e in ch.tolist() if e > low)
    out = []
    for b, e in found:
        if out and b <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((b, e))
    return out


# --- sorting by coordinate -------------------------------------------------------------------------------------------------

BGZF_BLOCK_DATA = 0xff00         # inflated bytes a written block holds at most (htslib's BGZF_BLOCK_SIZE)
DEVICE_MEMORY_SHARE = 0.8        # of the device's free memory a sort may plan with
_SORT_TABLE_BYTES = 56           # per record: offset, two (key, ordinal) pairs, length and destination
_ENDS_CHUNK = 1 << 20            # record ends fetched at a time
_DEFLATE_REGION = 2 * 65536      # device bytes the encoder needs for one block (slot and compacted copy)


def _header_data(path, verify=False):
    """
    (inflated bytes of the blocks the BAM header lies in, their number, header end, the bytes of the last of these blocks that
    belong to the header, [(SQ name, length)]).
    """
    data = bytearray()
    for k, (off, blk) in enumerate(iter_blocks(path)):
        start = len(data)
        data += _host_inflate(path, [(off, blk)], None, verify)[0]
        got = parse_header(data)
        if got is not None:
            return bytes(data), k + 1, got[0], got[0] - start, got[1]
    raise ValueError('{0}: BAM header cut short'.format(path))


def _header_lines(text):
    return text.rstrip(b'\x00').decode('latin-1').split('\n')


def sort_order(path):
    """The SO: value of the @HD line of a BAM file's header ('coordinate', 'queryname', 'unsorted', ...), or None without one."""
    data = _header_data(path)[0]
    l_text = struct.unpack_from('<i', data, 4)[0]
    first = _header_lines(data[8:8 + l_text])[0]
    if first.startswith('@HD'):
        for field in first.split('\t')[1:]:
            if field.startswith('SO:'):
                return field[3:]
    return None


def coordinate_header(header):
    """
    The bytes of a BAM header (magic to the end of the reference list) with the sort order of its text set to coordinate:
    the SO: field of the @HD line is replaced (appended when the line has none), a text without @HD line gets
    '@HD\\tVN:1.6\\tSO:coordinate' as its first line; other fields and lines, and the reference list, stay as they are.
    """
    l_text = struct.unpack_from('<i', header, 4)[0]
    lines = _header_lines(header[8:8 + l_text])
    if lines[0].startswith('@HD'):
        fields = lines[0].split('\t')
        if any(f.startswith('SO:') for f in fields[1:]):
            fields = [fields[0]] + ['SO:coordinate' if f.startswith('SO:') else f for f in fields[1:]]
        else:
            fields.append('SO:coordinate')
        lines[0] = '\t'.join(fields)
    else:
        lines.insert(0, '@HD\tVN:1.6\tSO:coordinate')
        if lines[-1] != '':                           # an empty text, or one that does not end its last line
            lines.append('')
    text = '\n'.join(lines).encode('latin-1')
    return header[:4] + struct.pack('<i', len(text)) + text + header[8 + l_text:]


def bgzf_compress(data, level=1):
    """One BGZF block holding `data` (at most 0xff00 bytes), deflated by zlib at `level`."""
    c = zlib.compressobj(int(level), zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    total = 18 + len(raw) + 8
    if len(data) > BGZF_BLOCK_DATA or total > 65536:
        raise ValueError('a BGZF block cannot hold {0} bytes'.format(len(data)))
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', total - 1) + raw +
            struct.pack('<II', zlib.crc32(data) & 0xffffffff, len(data)))


def bgzf_deflate(parts, device=None):
    """
    One whole BGZF block per `bytes` of `parts` (each at most 0xff00 bytes, else ValueError), deflated by the library's own
    DEFLATE encoder (csrc/dn_deflate.hip): on the host (device=None; no GPU needed) or on GPU `device`, one block per
    wavefront.  Both write the same bytes.  The counterpart of inflate_blocks.
    """
    parts = [bytes(p) for p in parts]
    n = len(parts)
    for k, part in enumerate(parts):
        if len(part) > BGZF_BLOCK_DATA:
            raise ValueError('part {0} holds {1} bytes; a BGZF block holds at most {2}'.format(k, len(part), BGZF_BLOCK_DATA))
    lens = np.array([len(part) for part in parts] + [0], np.int32)
    beg = np.zeros(n + 1, np.int64)
    np.cumsum(lens[:n], out=beg[1:])
    joined = b''.join(parts)
    data = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)
    lib = _lib.load()
    i64, i32, u8 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8
    cap = int(lib.dn_bgzf_deflate_bound(n, _ptr(lens, i32)))
    out, out_off = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.int64)
    args = (_ptr(data, u8), len(joined), n, _ptr(beg, i64), _ptr(lens, i32), _ptr(out, u8), cap, _ptr(out_off, i64))
    if device is None:
        _check(lib.dn_bgzf_deflate_host(*args), 'dn_bgzf_deflate_host')
    else:
        _check(lib.dn_bgzf_deflate(int(device), *(args + (None,))), 'dn_bgzf_deflate')
    raw = out[:int(out_off[n])].tobytes()
    return [raw[out_off[k]:out_off[k + 1]] for k in range(n)]


def _block_cuts(end_chunks):
    """
    [begin, end) of the blocks of a record stream whose records end at the offsets `end_chunks` yields (ascending int64
    arrays): a block takes whole records while they fit in BGZF_BLOCK_DATA bytes; a record longer than that is cut into
    blocks of its own.
    """
    cur, cand = 0, None
    for ends in end_chunks:
        i, n = 0, len(ends)
        while i < n:
            k = int(np.searchsorted(ends, cur + BGZF_BLOCK_DATA, side='right'))
            if k > i:
                cand, i = int(ends[k - 1]), k
                if k == n:
                    break                             # the next chunk's first records may still fit
            elif cand is None:
                end = int(ends[i])
                while cur < end:
                    nxt = min(cur + BGZF_BLOCK_DATA, end)
                    yield cur, nxt
                    cur = nxt
                i += 1
                continue
            yield cur, cand
            cur, cand = cand, None
    if cand is not None:
        yield cur, cand


def device_memory(device):
    """(free, total) bytes of GPU `device`."""
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _check(_lib.load().dn_bam_sort_device_memory(int(device), ctypes.byref(free), ctypes.byref(total)), 'dn_bam_sort_device_memory')
    return int(free.value), int(total.value)


def sort_bam(src, dst, device=None, n_jobs=1, level=1, window_bytes=256 << 20, segment_bytes=None, verify=False, overwrite=False,
             max_device_bytes=None, stats=None, deflate='zlib'):
    """
    Write the BAM file `src` sorted by coordinate to `dst` (what `samtools sort` is run for before an index can be made);
    returns dst.  The order is defined in include/degnorm_amd.h: ascending (refID, pos), records without a reference last,
    and records of equal (refID, pos) in the order of src -- which is not samtools' tie rule, so the two programs' outputs
    may differ in the order of such records.

    device=k: the BGZF blocks go to GPU k about window_bytes of inflated data at a time and are inflated there into one
    buffer that holds the whole record stream, which is framed, keyed, sorted (radix sort of key and ordinal), and copied
    record by record into a second buffer of the same size (csrc/dn_sort.hip); the sorted stream comes back window_bytes at
    a time.  The device must hold the stream twice: the need -- twice the inflated size, the largest window's compressed
    blocks and 56 bytes for each record, estimated at one per 128 bytes -- is checked before anything is uploaded against
    max_device_bytes, by default 0.8 of the memory hipMemGetInfo reports free, and a ValueError gives both figures.
    device=None: zlib inflates in n_jobs threads and the host build of the same source sorts (std::stable_sort); no GPU is
    needed.  Both write the same file.

    The header is copied with its @HD line's SO: set to coordinate (coordinate_header).  The output's blocks hold at most
    0xff00 inflated bytes and end where a record ends (a longer record gets blocks of its own), are deflated by zlib at
    `level` in n_jobs threads, and are written to dst + '.tmp', which becomes dst when complete.  verify: every block of src
    must have the CRC32 of its trailer.  Errors are ValueErrors that name src and the block's offset or the record's
    ordinal, the same from both paths, and leave neither dst nor dst + '.tmp' behind; FileExistsError when dst exists and
    overwrite is off.  stats, a dict, receives `inflate_device_ms`, `frame_device_ms`, `frame_fixups`, `sort_device_ms` (key
    pass, sort and scan), `gather_device_ms`, `records`, `bytes`, `windows`, `deflate_s`, `deflate_device_ms` (the encoder's
    kernels; 0 with zlib and on the host) and `out_bytes` (the bytes of the blocks that hold records: the file without its
    header blocks and its end-of-file block).

    deflate='native': the blocks are written by the library's own encoder (csrc/dn_deflate.hip, bgzf_deflate) in place of
    zlib; `level` applies to 'zlib' only.  On a device the sorted stream is deflated where it lies, about window_bytes of
    it at a time, and only the blocks come back; device=None runs the host build of the same source, and the header blocks
    go through it in both cases, so device=k and device=None write the same file.  The file differs from the 'zlib' one
    in its compressed bytes only: the blocks are cut at the same records.
    """
    if deflate not in ('zlib', 'native'):
        raise ValueError("deflate must be 'zlib' or 'native', not {0!r}".format(deflate))
    if os.path.exists(dst) and not overwrite:
        raise FileExistsError('{0} exists; pass overwrite=True to replace it'.format(dst))
    if not has_eof_block(src):
        raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(src))
    if segment_bytes is not None and int(segment_bytes) < 64:
        raise ValueError('segment_bytes must be at least 64, not {0}'.format(segment_bytes))
    window_bytes = max(int(256 << 20 if window_bytes is None else window_bytes), 1)
    lib = _lib.load()
    i64, i32, u8 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8
    n_jobs = max(int(n_jobs), 1)
    pool = ThreadPoolExecutor(max_workers=n_jobs) if n_jobs > 1 else None
    h = ctypes.c_void_p()
    tmp = dst + '.tmp'
    t = {'inflate_device_ms': 0.0, 'deflate_s': 0.0, 'windows': 0, 'deflate_device_ms': 0.0, 'out_bytes': 0}

    def call(rc, what):
        try:
            _check(rc, what)
        except ValueError as e:
            raise ValueError('{0}: {1}'.format(src, e))

    def window(batch, head_skip):
        t['windows'] += 1
        if device is None:
            data = b''.join(_host_inflate(src, batch, pool, verify))
            joined = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
            call(lib.dn_bam_sort_window_host(h, _ptr(joined, u8), len(data), int(head_skip)), 'dn_bam_sort_window_host')
            return
        args, status = _window_args([b for _, b in batch], verify, lambda crc: call(
            lib.dn_bam_sort_expect_crc(h, _ptr(crc, ctypes.c_uint32), len(crc)), 'dn_bam_sort_expect_crc'))
        ms = ctypes.c_double(0.0)
        call(lib.dn_bam_sort_window(h, *(args + (int(head_skip), _ptr(status, i32), ctypes.byref(ms)))), 'dn_bam_sort_window')
        t['inflate_device_ms'] += float(ms.value)
        _raise_block_status(src, batch, status)

    def ends_chunks(n_records):
        for first in range(0, n_records, _ENDS_CHUNK):
            n = min(_ENDS_CHUNK, n_records - first)
            ends = np.zeros(n, np.int64)
            call(lib.dn_bam_sort_ends(h, first, n, _ptr(ends, i64)), 'dn_bam_sort_ends')
            yield ends

    def deflated(parts):
        t0 = time.perf_counter()
        one = lambda d: bgzf_compress(d, level)                                  # noqa: E731
        out = list(pool.map(one, parts) if pool is not None else map(one, parts))
        t['deflate_s'] += time.perf_counter() - t0
        return out

    try:
        # the header, on zlib whatever the device: it may span several blocks; and the size of the whole stream
        data, head_blocks, header_end, head_skip, refs = _header_data(src, verify)
        _, _, isizes = bgzf_blocks(src)
        n_stream = int(isizes.sum()) - header_end
        n_comp_max, size, comp = 0, 0, 0
        for k in range(head_blocks - 1, len(isizes)):                            # the compressed bytes of the largest window
            size, comp = size + int(isizes[k]), comp + 65536
            if size >= window_bytes or k == len(isizes) - 1:
                n_comp_max, size, comp = max(n_comp_max, comp), 0, 0
        if device is not None:
            need = 2 * n_stream + n_comp_max + _SORT_TABLE_BYTES * (n_stream // 128 + 1)
            if deflate == 'native' and n_stream + 64 < _DEFLATE_REGION:      # too small to lend the encoder its slots
                need += _DEFLATE_REGION
            have = int(DEVICE_MEMORY_SHARE * device_memory(device)[0]) if max_device_bytes is None else int(max_device_bytes)
            if need > have:
                raise ValueError('{0}: sorting needs about {1} bytes of device memory ({2} bytes of records), {3} are allowed; '
                                 'a file that does not fit the device cannot be sorted here'.format(src, need, n_stream, have))
        call(lib.dn_bam_sort_create(-1 if device is None else int(device), len(refs), n_stream, int(segment_bytes or 0), window_bytes,
                                    ctypes.byref(h)), 'dn_bam_sort_create')
        # the first window starts inside the block in which the header ends, and counts that block whole
        for batch in _batched(itertools.islice(iter_blocks(src), head_blocks - 1, None), window_bytes):
            window(batch, head_skip)
            head_skip = 0
            del batch
        n_rec, n_bytes, fix = i64(0), i64(0), i64(0)
        ms = [ctypes.c_double(0.0) for _ in range(3)]
        call(lib.dn_bam_sort_finish(h, ctypes.byref(n_rec), ctypes.byref(n_bytes), ctypes.byref(fix), ctypes.byref(ms[0]), ctypes.byref(ms[1]),
                                    ctypes.byref(ms[2])), 'dn_bam_sort_finish')
        header = coordinate_header(data[:header_end])
        buf = {'lo': 0, 'data': b''}

        def stream(a, b):
            """Bytes [a, b) of the sorted stream; fetched window_bytes at a time, in ascending order."""
            if b > buf['lo'] + len(buf['data']):
                n = min(max(window_bytes, b - a), n_bytes.value - a)
                arr = np.zeros(max(n, 1), np.uint8)
                call(lib.dn_bam_sort_read(h, a, n, _ptr(arr, u8)), 'dn_bam_sort_read')
                buf['lo'], buf['data'] = a, arr[:n].tobytes()
            return buf['data'][a - buf['lo']:b - buf['lo']]

        def native(f, cuts):
            """The blocks of the ranges `cuts` of the sorted stream, deflated where the stream lies, to f."""
            t0 = time.perf_counter()
            beg = np.array([a for a, _ in cuts] + [0], np.int64)
            lens = np.array([b - a for a, b in cuts] + [0], np.int32)
            cap = int(lib.dn_bgzf_deflate_bound(len(cuts), _ptr(lens, i32)))
            out, out_off, dms = np.zeros(max(cap, 1), np.uint8), np.zeros(len(cuts) + 1, np.int64), ctypes.c_double(0.0)
            call(lib.dn_bam_sort_deflate(h, len(cuts), _ptr(beg, i64), _ptr(lens, i32), _ptr(out, u8), cap, _ptr(out_off, i64),
                                         ctypes.byref(dms)), 'dn_bam_sort_deflate')
            t['deflate_device_ms'] += float(dms.value)
            t['deflate_s'] += time.perf_counter() - t0
            t['out_bytes'] += int(out_off[len(cuts)])
            f.write(memoryview(out)[:int(out_off[len(cuts)])])

        head_parts = [header[a:a + BGZF_BLOCK_DATA] for a in range(0, len(header), BGZF_BLOCK_DATA)]
        with open(tmp, 'wb') as f:
            if deflate == 'native':
                for blk in bgzf_deflate(head_parts):
                    f.write(blk)
                cuts, size = [], 0
                for a, b in _block_cuts(ends_chunks(int(n_rec.value))):
                    cuts.append((a, b))
                    size += b - a
                    if size >= window_bytes:
                        native(f, cuts)
                        cuts, size = [], 0
                if cuts:
                    native(f, cuts)
            else:
                for blk in deflated(head_parts):
                    f.write(blk)
                parts = []
                for a, b in _block_cuts(ends_chunks(int(n_rec.value))):
                    parts.append(stream(a, b))
                    if len(parts) >= 64 * n_jobs:
                        for blk in deflated(parts):
                            t['out_bytes'] += len(blk)
                            f.write(blk)
                        parts = []
                for blk in deflated(parts):
                    t['out_bytes'] += len(blk)
                    f.write(blk)
            f.write(BGZF_EOF)
        os.replace(tmp, dst)
    finally:
        if h:
            lib.dn_bam_sort_destroy(h)
        if pool is not None:
            pool.shutdown()
        if os.path.exists(tmp):
            os.remove(tmp)
    if stats is not None:
        stats.update(t, frame_device_ms=float(ms[0].value), sort_device_ms=float(ms[1].value), gather_device_ms=float(ms[2].value),
                     frame_fixups=int(fix.value), records=int(n_rec.value), bytes=int(n_bytes.value))
    return dst
