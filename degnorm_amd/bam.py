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
A .bai ends at position 2^29: fmt='csi' builds the .csi index of (min_shift, depth) with the same builder, parse_csi /
write_index read and write its BGZF-compressed file, and read_index gives the reader what read_bai gives it, from either.

A file that is not sorted by coordinate -- an aligner's default output -- is sorted by sort_bam (csrc/dn_sort.hip): the whole
inflated record stream is inflated into one device buffer, framed, keyed, radix-sorted (stably: ties keep file order) and
copied record by record into a second buffer; the host cuts, deflates (zlib) and writes the blocks of the sorted file under a
header that says SO:coordinate.  device=None does the same with zlib and the host build of the same source.  With
deflate='native' the blocks are written by the library's own DEFLATE encoder instead (csrc/dn_deflate.hip, bgzf_deflate): on the
device the sorted stream is deflated where it lies, one block per wavefront, and only the blocks come back.

An aligner's text output -- a .sam file -- becomes a BAM file by sam_to_bam (csrc/dn_sam.hip): the host copies the '@' header
lines into the BAM header and hands the alignment lines over in windows cut at line ends; on the device one lane per line
measures its record, a scan places it and one lane per line writes it; the host cuts, deflates and writes the blocks, records
in input order.  device=None runs the host build of the same source; sam_records is the buffer-level call.

Every path that inflates takes verify=True: the inflated bytes of each BGZF block are then compared with the CRC32 of its
trailer -- zlib.crc32 where zlib inflates, the wavefront that inflates the block where the device does -- and a block that
differs is a ValueError naming the file and the block's offset.  verify_bgzf checks a whole file that way (bgzip -t).

The four drivers -- the reader's device_rows, build_index, sort_bam and verify_bgzf -- take their blocks from one window feed
(_WindowFeed): it cuts the file, or one reference's index range, into windows by one rule (_window_cuts) and yields _Window
items that inflate themselves on the host (_host_inflate, one error text for every driver) or go to a handle as they are.
The handles that take windows have one shape (_WindowHandle): DeviceRows, _IndexBuilder (dn_bai_*) and _Sorter (dn_bam_sort_*).
"""
import ctypes
import itertools
import logging
import os
import pickle as pkl
import struct
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, gz
from ._lib import _check, _p as _ptr
from .reads import (BamReadsProcessor, Annotation, STRANDED, STRANDS, check_coverage_call, check_strand, check_stranded,
                    coverage_outputs, reads_frame)

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


def _out_offsets(isize, n):
    """
    Where the data of n blocks with these ISIZEs begins and ends when it is written back to back (n + 1 int64 offsets), or
    (None, k) when block k, the largest, claims more than the 65536 bytes the library's decoder takes: the caller names it.
    """
    k = int(isize[:n].argmax()) if n else 0
    if n and int(isize[k]) > 65536:
        return None, k
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(isize[:n], out=out_off[1:])
    return out_off, None


def inflate_blocks(blocks, device=None, verify=False):
    """
    The data of whole BGZF blocks (as iter_blocks yields them), inflated by the library's own DEFLATE decoder: on the host
    (device=None; no GPU needed) or on GPU `device`, one block per wavefront.  ValueError names the first block that does
    not decode or (verify) whose bytes do not have the CRC32 of its trailer.
    """
    blocks = list(blocks)
    n = len(blocks)
    comp, n_comp, pay_off, pay_len, isize = _block_layout(blocks)
    out_off, big = _out_offsets(isize, n)
    if big is not None:
        raise ValueError('BGZF block {0} claims an inflated size of {1} bytes'.format(big, int(isize[big])))
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


def _isize(blk):
    """The ISIZE of a whole BGZF block: the inflated size its trailer claims."""
    return struct.unpack_from('<I', blk, len(blk) - 4)[0]


def _window_cuts(sizes, window_bytes, size0=0):
    """
    The cut rule of every window loop: the number of items of each window over items of these sizes, in order.  A window ends
    with the item that brings its size to window_bytes; the first window starts counting at size0 (negative: bytes of its first
    item that are not its), every later one at 0, and the last takes what is left.
    """
    n, size = 0, size0
    for s in sizes:
        n, size = n + 1, size + s
        if size >= window_bytes:
            yield n
            n, size = 0, 0
    if n:
        yield n


def _batched(blocks, window_bytes, size=0, weigh=lambda ob: _isize(ob[1])):
    """
    Lists of the (file offset, block) pairs that `blocks` yields, cut by _window_cuts on the blocks' ISIZEs (size: its size0;
    weigh: the size of an item of another kind).  A loop over whole files drops its list (`del batch`) when it is done with it:
    otherwise the blocks of one window stay allocated while the next window's are read, which costs more than the marshalling of
    a window does.  This generator keeps no reference to a list it has yielded.
    """
    blocks, weighed = itertools.tee(blocks)
    for n in _window_cuts(map(weigh, weighed), window_bytes, size):
        yield list(itertools.islice(blocks, n))


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


def _host_inflate(path, batch, pool, verify=False):
    """
    The data of the blocks of batch, in file order, by zlib (in pool, when there is one; verify: and their CRC32s by
    zlib.crc32, in the same pool).  The first block that fails is a ValueError naming the file and its offset with the text of the
    library's own decoder; one whose data does not have the CRC32 of its trailer is a BgzfCrcError (a ValueError).
    """
    blocks = [b for _, b in batch]
    one = (lambda blk: inflate_block(blk, True)) if verify else inflate_block
    data = []
    try:
        for d in (pool.map(one, blocks) if pool is not None else map(one, blocks)):      # in file order: the first bad block raises
            data.append(d)
    except BgzfCrcError:                                 # the blocks before it were good: this is the one, whatever its ISIZE
        raise BgzfCrcError(_block_error(path, batch[len(data)][0], INFLATE_E_CRC))
    except (zlib.error, ValueError, struct.error) as e:  # the library's host decoder finds the block and the words
        args, isize, status = _block_args(blocks)
        out_off, big = _out_offsets(isize, len(blocks))
        if big is None:
            out = np.zeros(int(out_off[-1]) + 1, np.uint8)
            crc = _ptr(block_crcs(blocks), ctypes.c_uint32) if verify else None
            args += (_ptr(out_off, ctypes.c_int64), _ptr(out, ctypes.c_uint8), _ptr(status, ctypes.c_int32), crc)
            _check(_lib.load().dn_bgzf_inflate_check_host(*args), 'dn_bgzf_inflate_check_host')
            _raise_block_status(path, batch, status)
        raise ValueError('{0}: a BGZF block at or after byte {1} does not inflate: {2}'.format(path, batch[0][0], e))
    return data


# --- the window feed -----------------------------------------------------------------------------------------------------

class _Closing(object):
    """The with statement for an object with close()."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _Window(object):
    """
    One window of a _WindowFeed: `batch`, the (file offset, block) pairs of whole BGZF blocks in file order; head_skip, the
    bytes of the first block's data that are not the window's; tail_keep, the bytes of the last block's data that are (-1: all
    of them).  verify is the feed's.
    """

    def __init__(self, feed, batch, head_skip=0, tail_keep=-1):
        self.feed, self.batch, self.head_skip, self.tail_keep, self.verify = feed, batch, int(head_skip), int(tail_keep), feed.verify

    @property
    def blocks(self):
        return [blk for _, blk in self.batch]

    def host_data(self):
        """The data of every block, whole, by zlib in the feed's pool (_host_inflate: its errors name the file and the block)."""
        return _host_inflate(self.feed.path, self.batch, self.feed.pool, self.verify)

    def host_bytes(self):
        """The window's bytes: the blocks' data joined, without what head_skip and tail_keep leave out."""
        data = self.host_data()
        if self.tail_keep >= 0:
            data[-1] = data[-1][:self.tail_keep]
        if self.head_skip:
            data[0] = data[0][self.head_skip:]
        return b''.join(data)

    def check(self, status):
        """ValueError naming the file and the first block whose status, as a device entry point filled it, is not 0."""
        _raise_block_status(self.feed.path, self.batch, status)


class _WindowFeed(_Closing):
    """
    The BGZF windows of one file, for every driver that reads one (the reader, build_index, sort_bam, verify_bgzf): the path,
    window_bytes (None: 256 MiB), verify, and the zlib thread pool of a caller that inflates on the host (n_jobs > 1; a caller
    that inflates on the device passes 1), shut down by close() or the with statement.  Refuses a file without BGZF's
    end-of-file block.  whole() and reference() yield _Window items cut by _window_cuts.
    """

    def __init__(self, path, window_bytes=None, verify=False, n_jobs=1):
        if not has_eof_block(path):
            raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(path))
        self.path, self.verify = path, bool(verify)
        self.window_bytes = max(int(256 << 20 if window_bytes is None else window_bytes), 1)
        self.pool = ThreadPoolExecutor(max_workers=int(n_jobs)) if int(n_jobs) > 1 else None

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
            self.pool = None

    def header(self):
        """_header_data of the file: on zlib whatever the device, since the header may span several blocks."""
        return _header_data(self.path, self.verify)

    def whole(self, first=0, size0=0, head_skip=0):
        """
        The windows of the whole file from block `first` on; the first window leaves out head_skip bytes of that block's data and
        starts counting at size0.
        """
        return self._windows(itertools.islice(iter_blocks(self.path), first, None), size0, head_skip)

    def reference(self, rng):
        """
        The windows of the blocks that hold the [begin, end) virtual offsets rng (reference_range; None: no window): the first
        starts at begin's offset into its block, the last ends at end's.
        """
        if rng is None:
            return iter(())
        cbeg, ubeg, cend, uend = rng[0] >> 16, rng[0] & 0xffff, rng[1] >> 16, rng[1] & 0xffff
        in_range = itertools.takewhile(lambda ob: ob[0] < cend or (ob[0] == cend and uend > 0), iter_blocks(self.path, cbeg))
        return self._windows(in_range, 0, ubeg, cend, uend)

    def _windows(self, blocks, size0, head_skip, cend=-1, uend=-1):
        for batch in _batched(blocks, self.window_bytes, size0):
            win = _Window(self, batch, head_skip, uend if batch[-1][0] == cend else -1)
            del batch                                    # the item holds the only reference to its blocks
            yield win
            # the caller is done with the window: its blocks go here, before those of the next window are read (_batched)
            win.batch, head_skip = None, 0


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
    return _header_data(path, verify)[4]


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


def pseudo_bin(depth):
    """The id of the pseudo-bin of an index of `depth` levels: 37450 at the .bai's depth 5."""
    return ((1 << 3 * (int(depth) + 1)) - 1) // 7 + 1


def _csi_bytes(path, raw):
    """The inflated bytes of a .csi file (a BGZF stream; any sequence of gzip members is read), which start with the magic."""
    out, rest = [], raw
    try:
        while rest:
            d = zlib.decompressobj(31)
            out.append(d.decompress(rest))
            if not d.eof:
                raise ValueError('{0}: truncated .csi index (its last gzip member is cut short)'.format(path))
            rest = d.unused_data
    except zlib.error as e:
        raise ValueError('{0} is not a .csi index ({1})'.format(path, e))
    data = b''.join(out)
    if data[:4] != b'CSI\x01':
        raise ValueError('{0} is not a .csi index'.format(path))
    return data


def _csi_fields(path, b):
    """(min_shift, depth, aux, [per reference [(bin, loffset, (n, 2) chunks)] in file order], n_no_coor or None)."""
    try:
        min_shift, depth, l_aux = struct.unpack_from('<iii', b, 4)
        if l_aux < 0 or 16 + l_aux + 4 > len(b):
            raise ValueError('l_aux = {0}'.format(l_aux))
        aux = bytes(b[16:16 + l_aux])
        p = 16 + l_aux
        n_ref = struct.unpack_from('<i', b, p)[0]
        p += 4
        refs = []
        for _ in range(n_ref):
            n_bin = struct.unpack_from('<i', b, p)[0]
            p += 4
            bins = []
            for _ in range(n_bin):
                bin_id, loffset, n_chunk = struct.unpack_from('<IQi', b, p)
                p += 16
                bins.append((bin_id, loffset, np.frombuffer(b, dtype='<u8', count=2 * n_chunk, offset=p).reshape(n_chunk, 2).astype(np.uint64)))
                p += 16 * n_chunk
            refs.append(bins)
    except (struct.error, ValueError) as e:
        raise ValueError('{0}: truncated .csi index ({1})'.format(path, e))
    return min_shift, depth, aux, refs, struct.unpack_from('<Q', b, p)[0] if len(b) >= p + 8 else None


def read_index(path):
    """
    What the reader needs of an index file, as read_bai gives it.  A file that starts with the gzip magic is a .csi index
    (a BGZF stream whose inflated bytes start with 'CSI\\1'; ValueError otherwise); any other file goes to read_bai.
    """
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:2] != b'\x1f\x8b':
        return read_bai(path)
    min_shift, depth, _, bins, n_no_coor = _csi_fields(path, _csi_bytes(path, raw))
    refs = []
    for ref_bins in bins:
        pseudo, lo, hi = None, None, None
        for bin_id, _, ch in ref_bins:
            if bin_id == pseudo_bin(depth):
                pseudo = tuple(int(x) for x in ch.reshape(-1)[:4])
            elif len(ch):
                lo = int(ch[:, 0].min()) if lo is None else min(lo, int(ch[:, 0].min()))
                hi = int(ch[:, 1].max()) if hi is None else max(hi, int(ch[:, 1].max()))
        refs.append({'n_bin': len(ref_bins), 'pseudo': pseudo, 'chunk_min': lo, 'chunk_max': hi})
    return refs, n_no_coor


def reference_range(ref):
    """[begin, end) virtual offsets of one reference's records from its .bai entry, or None when it has no reads."""
    if ref['pseudo'] is not None:
        return ref['pseudo'][0], ref['pseudo'][1]
    if ref['chunk_min'] is None:
        return None
    return ref['chunk_min'], ref['chunk_max']


# --- framing and the device row store ------------------------------------------------------------------------------------

def _segment_arg(segment_bytes):
    """The segment size of the framing as the library takes it: 0, its default, for None; ValueError below 64."""
    if segment_bytes is not None and int(segment_bytes) < 64:
        raise ValueError('segment_bytes must be at least 64, not {0}'.format(segment_bytes))
    return int(segment_bytes or 0)


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
    seg = _segment_arg(segment_bytes or None)            # 0 is the library's default here too
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


PAIRINGS = ('name', 'flag', 'auto')


def check_read_options(pairing, exclude_flags, require_flags, min_mapq, modes=PAIRINGS):
    """ValueError unless pairing is one of `modes`, the two masks are ints in 0 .. 0xffff and min_mapq is an int in 0 .. 255."""
    if pairing not in modes:
        raise ValueError('pairing must be {0}, not {1!r}'.format(' or '.join(repr(m) for m in modes), pairing))
    for name, v, top in (('exclude_flags', exclude_flags, 0xffff), ('require_flags', require_flags, 0xffff), ('min_mapq', min_mapq, 255)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= top:
            raise ValueError('{0} must be an integer in 0 .. {1}, not {2!r}'.format(name, top, v))


class _WindowHandle(_Closing):
    """
    What the library handles that take BGZF windows share -- DeviceRows (dn_bam_rows_*) here, _IndexBuilder (dn_bai_*) and _Sorter
    (dn_bam_sort_*) below.  Each creates its handle `h` and names its `unit`; from here come close() (<unit>_destroy),
    expect_crc() (<unit>_expect_crc), the arguments of the unit's device entry points, and call(), which names the file of a
    handle that has a `path` in front of a ValueError.
    """
    unit, path = None, None

    def close(self):
        if self.h:
            getattr(self.lib, self.unit + '_destroy')(self.h)
            self.h = ctypes.c_void_p()

    def call(self, rc, what):
        try:
            _check(rc, what)
        except ValueError as e:
            raise e if self.path is None else ValueError('{0}: {1}'.format(self.path, e))

    def expect_crc(self, crc):
        """<unit>_expect_crc: the next window inflated on the device checks its blocks against these CRC32s (one per block)."""
        crc, what = np.ascontiguousarray(crc, dtype=np.uint32), self.unit + '_expect_crc'
        self.call(getattr(self.lib, what)(self.h, _ptr(crc, ctypes.c_uint32) if len(crc) else None, len(crc)), what)

    def window_args(self, blocks, verify=False):
        """_window_args of a window's blocks; verify: their CRC32s are announced to this handle first."""
        return _window_args(blocks, verify, self.expect_crc)


class DeviceRows(_WindowHandle):
    """The device-resident rows of one chromosome (dn_bam_rows): kept records in file order."""
    unit = 'dn_bam_rows'

    def __init__(self, tid, unique_alignment, paired, device=None, pairing='name', exclude_flags=0, require_flags=0, min_mapq=0,
                 stranded='no'):
        """
        pairing: how a paired store tells mates -- 'name' (qname_unpaired) or 'flag' (FLAG bits and mate positions; the
        rule is in include/degnorm_amd.h).  exclude_flags, require_flags, min_mapq: the read filters, 0 for none.  With
        the defaults this is the store of dn_bam_rows_create.  stranded 'forward' or 'reverse': the store also keeps the
        sense of every row (dn_bam_rows_set_stranded), for coverage(..., strand=).
        """
        self.h = ctypes.c_void_p()
        check_read_options(pairing, exclude_flags, require_flags, min_mapq, modes=('name', 'flag'))
        self.stranded = check_stranded(stranded)
        self._paired_rows = -1                           # the rows there were at the last pair()
        self.lib = _lib.load()
        self.paired = bool(paired)
        self.by_flag = self.paired and pairing == 'flag'
        self.filtered = bool(exclude_flags or require_flags or min_mapq)
        dev = int(os.environ.get('LOCAL_RANK', 0)) if device is None else int(device)
        if self.by_flag or self.filtered:
            opt = _lib.BamRowsOptions(1 if self.by_flag else 0, int(exclude_flags), int(require_flags), int(min_mapq))
            _check(self.lib.dn_bam_rows_create_with(dev, int(tid), 1 if unique_alignment else 0, 1 if paired else 0, ctypes.byref(opt),
                                                    ctypes.byref(self.h)), 'dn_bam_rows_create_with')
        else:
            _check(self.lib.dn_bam_rows_create(dev, int(tid), 1 if unique_alignment else 0, 1 if paired else 0,
                                               ctypes.byref(self.h)), 'dn_bam_rows_create')
        if self.stranded != 'no':
            _check(self.lib.dn_bam_rows_set_stranded(self.h, STRANDED.index(self.stranded)), 'dn_bam_rows_set_stranded')

    def __del__(self):
        self.close()

    def append(self, buf, rec_off):
        if len(rec_off) == 0:
            return
        a = np.frombuffer(buf, dtype=np.uint8)
        _check(self.lib.dn_bam_rows_append(self.h, _ptr(a, ctypes.c_uint8), len(buf), _ptr(rec_off, ctypes.c_int64),
                                           len(rec_off)), 'dn_bam_rows_append')

    def inflate(self, carry, blocks, head_skip, tail_keep, verify=False):
        """
        dn_bam_rows_inflate: the next window (carry + the inflated blocks, trimmed) built on the device.  Returns a view of
        the library's host copy of it (valid until the next call), the status of every block and the kernel's ms.
        verify: every block, all of it, must have the CRC32 of its trailer (status 8 otherwise).
        """
        args, status = self.window_args(blocks, verify)
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
        args, status = self.window_args(blocks, verify)
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

    def fetch_mates(self):
        """(flag uint16, mapq uint8, next_pos int32) of the rows of a store that pairs by FLAG (ValueError for any other)."""
        n = self.info()[0]
        flag, mapq, pnext = np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32)
        _check(self.lib.dn_bam_rows_fetch_mates(self.h, _ptr(flag, ctypes.c_uint16), _ptr(mapq, ctypes.c_uint8), _ptr(pnext, ctypes.c_int32)),
               'dn_bam_rows_fetch_mates')
        return flag[:n], mapq[:n], pnext[:n]

    def fetch_sense(self):
        """The sense of the rows of a stranded store as bytes '+' / '-' (uint8; ValueError for any other store)."""
        n = self.info()[0]
        sense = np.zeros(max(n, 1), np.uint8)
        _check(self.lib.dn_bam_rows_fetch_sense(self.h, _ptr(sense, ctypes.c_uint8)), 'dn_bam_rows_fetch_sense')
        return sense[:n]

    def dropped(self):
        """Records of the windows so far that (exclude_flags / require_flags, min_mapq, the FLAG rule's candidate test) dropped."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib.dn_bam_rows_dropped(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), 'dn_bam_rows_dropped')
        return int(a.value), int(b.value), int(c.value)

    def pair(self, fetch=False):
        """
        dn_bam_rows_pair: pair the mates on the device and keep the result there.  Rows go in ascending qname_unpaired order,
        equal keys in file order: np.argsort(self.keys(), kind='stable').  A store that pairs by FLAG orders them by the whole
        name, then by the two mate coordinates (mate_rows on the host).  Returns (order int32, pair_id int32, number of ids,
        device ms) with fetch=True, (None, None, number of ids, device ms) otherwise.
        """
        n = self.info()[0] if fetch else 0
        order = np.zeros(max(n, 1), np.int32) if fetch else None
        pair_id = np.zeros(max(n, 1), np.int32) if fetch else None
        n_ids, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _check(self.lib.dn_bam_rows_pair(self.h, _ptr(order, ctypes.c_int32), _ptr(pair_id, ctypes.c_int32), ctypes.byref(n_ids),
                                         ctypes.byref(ms)), 'dn_bam_rows_pair')
        self._paired_rows = self.info()[0]               # rows appended later end the pairing
        if fetch:
            return order[:n], pair_id[:n], int(n_ids.value), float(ms.value)
        return None, None, int(n_ids.value), float(ms.value)

    def coverage(self, ann, pair='host', strand=None):
        """
        dn_bam_rows_coverage: the outputs of reads.device_read_coverage for the stored rows.  A paired store's mates are
        paired on the host in the reference's order (pair_order; pair='host') or on the device with equal keys in file order
        (self.pair(); pair='device'), which moves no keys to the host; self.pair_ms is then the pairing's device ms.  A store
        that pairs by FLAG is always paired on the device, whatever `pair` says.
        strand '+' or '-' (a stranded store only): dn_bam_rows_coverage_strand on the rows of that sense, with ann the
        annotation of that strand.  Such a call always pairs on the device, and the calls of both strands share one pairing
        (pair_ms is 0.0 for the call that found it there).
        """
        if pair not in ('host', 'device'):
            raise ValueError("pair must be 'host' or 'device', not {0!r}".format(pair))
        if strand is not None and self.stranded == 'no':
            raise ValueError("coverage(strand=) takes a store created with stranded='forward' or 'reverse'")
        sel = () if strand is None else (check_strand(strand),)
        order, pair_id, n_ids = None, None, 0
        self.pair_ms = 0.0
        if self.paired and sel:
            if self.info()[0] != self._paired_rows:
                self.pair_ms = self.pair()[3]
        elif self.paired and (pair == 'device' or self.by_flag):
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
        call = self.lib.dn_bam_rows_coverage_strand if sel else self.lib.dn_bam_rows_coverage
        rc = call(*((self.h,) + sel + (_ptr(order, i32), _ptr(pair_id, i32), int(n_ids),
                                      ann.chrom_len, ann.keep_lo, ann.keep_hi,
                                      len(ann.exon_iv), _ptr(ann.exon_iv, i64),
                                      len(ann.group_iv), _ptr(ann.group_iv, i64), _ptr(ann.group_gene_off, i32),
                                      _ptr(ann.ol_gene, i32), _ptr(ann.ol_gs0, i64), _ptr(ann.ol_cov_off, i64),
                                      _ptr(ann.ol_exon_off, i32), _ptr(ann.ol_exon, i64),
                                      len(ann.iso_iv), _ptr(ann.iso_iv, i64), _ptr(ann.iso_gene, i32),
                                      len(ann.iso_union), _ptr(ann.iso_union, i64),
                                      n_genes, _ptr(counts, i64), _ptr(ol_cov, i64), cap, ctypes.byref(nnz),
                                      _ptr(csr_idx, i32), _ptr(csr_val, i64), ctypes.byref(n_iso_reads), ctypes.byref(ms))))
        check_coverage_call(rc, 'dn_bam_rows_coverage_strand' if sel else 'dn_bam_rows_coverage')
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


def mate_rows(names, pos, next_pos, flag):
    """
    The order and pair ids of DeviceRows.pair() for a store that pairs by FLAG, for rows in file order with these names (an
    S-dtype array or a list of bytes), positions, mate positions and FLAGs, computed by the library's host build of the same
    passes (dn_bam_mate_host; no device needed): (order int32, pair_id int32, number of ids).  Rows go by name, then by
    (uint32) (pos_first + 1), then by (uint32) (pos_last + 1), rows of equal key in file order; a row with 0x40 set has
    pos_first = pos and pos_last = next_pos, any other row the other way round.
    """
    names = [bytes(k) for k in (names.tolist() if isinstance(names, np.ndarray) else names)]
    n = len(names)
    pos, next_pos, flag = (np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in ((pos, np.int64), (next_pos, np.int32), (flag, np.uint16)))
    if not len(pos) == len(next_pos) == len(flag) == n:
        raise ValueError('mate_rows: names, pos, next_pos and flag must have one entry per row')
    name_len = np.array([len(k) for k in names] or [0], dtype=np.int32)
    name_beg = np.zeros(max(n, 1), dtype=np.int64)
    if n > 1:
        np.cumsum(name_len[:-1], out=name_beg[1:n])
    blob = b''.join(names)
    chars = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)
    if n == 0:
        pos, next_pos, flag = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.uint16)
    order, pair_id = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    n_ids = ctypes.c_int64(0)
    _check(_lib.load().dn_bam_mate_host(n, _ptr(name_beg, ctypes.c_int64), _ptr(name_len, ctypes.c_int32), _ptr(chars, ctypes.c_uint8),
                                        _ptr(pos, ctypes.c_int64), _ptr(next_pos, ctypes.c_int32), _ptr(flag, ctypes.c_uint16),
                                        _ptr(order, ctypes.c_int32), _ptr(pair_id, ctypes.c_int32), ctypes.byref(n_ids)), 'dn_bam_mate_host')
    return order[:n], pair_id[:n], int(n_ids.value)


def cigar_strings(op_beg, n_op, ops):
    """pysam's cigarstring of every row (None for a row without ops)."""
    lens, codes = (ops >> 4).tolist(), (ops & 15).tolist()
    tok = [str(l) + CIGAR_OPS[c] if c < 9 else str(l) + '?' for l, c in zip(lens, codes)]
    return [''.join(tok[b:b + k]) if k else None for b, k in zip(op_beg.tolist(), n_op.tolist())]


# --- the processor -------------------------------------------------------------------------------------------------------

class NativeBamReadsProcessor(BamReadsProcessor):
    index_extensions = ('.bai', '.csi')          # read_index tells them apart by their first bytes

    def __init__(self, bam_file, index_file, chroms=None, n_jobs=1, output_dir=None, unique_alignment=True, verbose=True,
                 window_bytes=256 << 20, inflate='host', frame='host', frame_segment_bytes=None, verify=False, pair='host',
                 pairing='name', exclude_flags=0, require_flags=0, min_mapq=0, stranded='no'):
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
        pairing says which records form a fragment.  'name' (the default, the reference's rule): the file is paired when the
        first 301 names of the first chromosome end in exactly .1 and .2, and mates share the name up to its last '.'.
        'flag': it is paired when one of those 301 records has FLAG 0x1, and mates are told by FLAG bits and mate positions
        (include/degnorm_amd.h), always on the device whatever `pair` says -- what HISAT2, STAR, BWA and Bowtie2 write.
        'auto': the name rule if it says paired, otherwise the FLAG rule, otherwise single-end; self.pairing_rule is then
        the rule in force.  exclude_flags / require_flags / min_mapq drop records as samtools view -F / -f / -q does, before
        every other rule; all 0 by default.  self.dropped sums what each rule dropped.
        stranded 'forward' or 'reverse' counts reads by strand (the rule: include/degnorm_amd.h, "Strand-specific counting"):
        the gene tables then carry a `strand` column of '+' and '-', every chromosome is two passes over one row store, each
        strand's genes with their own overlap structure and the rows of that sense, mates are paired on the device whatever
        `pair` says, and the chromosome's files are read_counts_<s>_<chr>.csv, overlap_coverage_<s>_<chr>.pkl and
        chrom_coverage_<s>_<chr>_plus.npz / _minus.npz.  'no' (the default) is the processor without the option.
        """
        check_read_options(pairing, exclude_flags, require_flags, min_mapq)
        self.stranded = check_stranded(stranded)
        self.pairing, self.pairing_rule = pairing, 'flag' if pairing == 'flag' else 'name'
        self.exclude_flags, self.require_flags, self.min_mapq = int(exclude_flags), int(require_flags), int(min_mapq)
        self.dropped = {'flags': 0, 'mapq': 0, 'not_candidate': 0}
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
            self._refs = self._feed(False).header()[4]
            self._index, _ = read_index(self.index_filename)
            if len(self._index) != len(self._refs):
                raise ValueError('{0} indexes {1} references, {2} has {3}'.format(
                    self.index_filename, len(self._index), self.filename, len(self._refs)))
            self._tid = {name: k for k, (name, _) in enumerate(self._refs)}

    def _reference_lengths(self):
        self._load()
        return {name: length for name, length in self._refs}

    def _feed(self, host, window_bytes=None):
        """The file's window feed (a context manager); host: with the pool of n_jobs threads that inflates its blocks here."""
        return _WindowFeed(self.filename, window_bytes or self.window_bytes, self.verify, self.n_jobs if host else 1)

    def _chrom_windows(self, feed, chrom):
        """The feed's windows over chrom's index range."""
        self._load()
        return feed.reference(reference_range(self._index[self._tid[chrom]]))

    def _batches(self, chrom, window_bytes=None):
        """The windows over chrom's index range, for a caller that only walks them: no pool."""
        return self._chrom_windows(self._feed(False, window_bytes), chrom)

    def windows(self, chrom, window_bytes=None):
        """
        Inflated bytes of the blocks that hold chrom's records, about window_bytes at a time; a record may be cut at the
        end of one window and continue in the next.  Adds host inflate seconds to self.timing['inflate_s'].
        """
        self._load()
        with self._feed(True, window_bytes) as feed:
            for win in self._chrom_windows(feed, chrom):
                yield self._inflate(win)

    def _inflate(self, win):
        t0 = time.perf_counter()
        out = win.host_bytes()
        self.timing['inflate_s'] = self.timing.get('inflate_s', 0.0) + time.perf_counter() - t0
        return out

    def _leading_records(self, chrom):
        """(query names, FLAGs) of the first 301 records of chrom, in file order, unfiltered."""
        self._load()
        names, flags, carry, last = [], [], b'', _INT32_MIN
        for win in self.windows(chrom, window_bytes=1 << 20):
            data = carry + win
            off, used, last = frame_records(data, self._tid[chrom], last)
            for o in off.tolist():
                l_name = data[o + 12]
                names.append(data[o + 36:o + 35 + l_name].decode('ascii', 'replace'))
                flags.append(data[o + 18] | data[o + 19] << 8)
                if len(names) > 300:
                    return names, flags
            carry = data[used:]
        return names, flags

    def _leading_query_names(self, chrom):
        return self._leading_records(chrom)[0]

    def determine_if_paired(self):
        """
        self.paired and self.pairing_rule by self.pairing: the reference's rule on the leading names ('name'), any leading
        record with FLAG 0x1 ('flag'), or the first of the two that says paired ('auto').
        """
        if self.pairing == 'name':
            return super(NativeBamReadsProcessor, self).determine_if_paired()
        self.paired = False
        names, flags = self._leading_records(self.chroms[0])
        by_name = set(x.split('.')[-1] for x in names) == {'1', '2'}
        by_flag = any(f & 0x1 for f in flags)
        if self.pairing == 'auto' and by_name:
            self.pairing_rule, self.paired = 'name', True
        else:
            self.pairing_rule, self.paired = 'flag' if by_flag or self.pairing == 'flag' else 'name', by_flag

    def device_rows(self, chrom, device=None):
        """
        The chromosome's kept records as a DeviceRows store (file order): one loop over the windows of its index range, in
        which inflate and frame choose the store's entry point.  The record a window's end cuts is carried to the next
        window: its bytes here, or (inflate and frame both 'device') their number, while the bytes wait on the device.
        """
        self._load()
        tid, t = self._tid[chrom], self.timing
        host_inflate, host_frame = self.inflate == 'host', self.frame == 'host'
        rows = DeviceRows(tid, self.unique_alignment, self.paired, device, self.pairing_rule, self.exclude_flags, self.require_flags,
                          self.min_mapq, self.stranded)
        carry, last = b'', _INT32_MIN
        calls = 0.0                         # frame='device': seconds in the library's one call per window; it splits them (frame_info)

        def add(key, value):
            t[key] = t.get(key, 0.0) + value

        try:
            if not host_frame:
                rows.frame_segment(self.frame_segment_bytes)
            try:
                with self._feed(host_inflate) as feed:
                    for win in self._chrom_windows(feed, chrom):
                        if host_inflate:
                            data = self._inflate(win)
                            data = carry + data if carry else data
                        t0 = time.perf_counter()
                        if host_inflate and host_frame:
                            off, used, last = frame_records(data, tid, last)
                            t1 = time.perf_counter()
                            rows.append(data, off)
                            add('frame_s', t1 - t0)
                            add('decode_s', time.perf_counter() - t1)
                            carry = data[used:]
                        elif host_frame:
                            data, status, ms = rows.inflate(carry, win.blocks, win.head_skip, win.tail_keep, self.verify)
                            t1 = time.perf_counter()
                            win.check(status)
                            off, used, last = frame_records(data, tid, last)
                            t2 = time.perf_counter()
                            rows.append_resident(off)
                            add('inflate_s', t1 - t0)
                            add('inflate_device_ms', ms)
                            add('frame_s', t2 - t1)
                            add('decode_s', time.perf_counter() - t2)
                            carry = data[used:].tobytes()
                        elif host_inflate:
                            used = rows.append_framed(data)
                            calls += time.perf_counter() - t0
                            carry = data[used:]
                        else:
                            status, carry, ms, _ = rows.inflate_framed(win.blocks, win.head_skip, win.tail_keep, self.verify)
                            t1 = time.perf_counter()
                            win.check(status)
                            add('inflate_device_ms', ms)
                            calls += t1 - t0
                if carry:
                    raise ValueError('{0}: a record of {1} is cut short at the end of its index range'.format(self.filename, chrom))
                if rows.filtered or rows.by_flag:
                    rows.n_dropped = dict(zip(('flags', 'mapq', 'not_candidate'), rows.dropped()))
                    for k, v in rows.n_dropped.items():
                        self.dropped[k] += v
            finally:
                if not host_frame:
                    _, fixups, ms, decode_ms = rows.frame_info()
                    add('frame_device_ms', ms)
                    t['frame_fixups'] = t.get('frame_fixups', 0) + fixups
                    add('decode_s', 1e-3 * decode_ms)
                    # what is left of the calls: the copy of the window (inflate='host') or of its blocks and their inflate ('device')
                    add('inflate_s' if self.inflate == 'device' else 'upload_s', max(calls - 1e-3 * (ms + decode_ms), 0.0))
        except Exception:
            rows.close()
            raise
        return rows

    def load_chromosome_reads(self, chrom):
        """
        The reference's DataFrame of one chromosome's reads (`qname`, `pos`, `cigar`, plus `qname_unpaired` and sorted by
        it when paired), built from the device-decoded rows.  A file paired by FLAG gives the candidate rows in file order
        with `qname`, `pos`, `cigar`, `flag`, `mapq`, `pnext`, and `qname_unpaired` equal to `qname`.  A stranded processor
        adds `sense`, '+' or '-', the strand each row's fragment came from.
        """
        rows = self.device_rows(chrom)
        try:
            pos, op_beg, n_op, ops, name_beg, name_len, names = rows.fetch()
            mates = rows.fetch_mates() if rows.by_flag else None
            sense = rows.fetch_sense() if self.stranded != 'no' else None
        finally:
            rows.close()
        nb = names.tobytes()
        qname = [nb[b:b + k].decode('ascii', 'replace') for b, k in zip(name_beg.tolist(), name_len.tolist())]
        df = reads_frame(list(zip(qname, pos.tolist(), cigar_strings(op_beg, n_op, ops))), self.paired and mates is None)
        if mates is not None:
            df['flag'], df['mapq'], df['pnext'] = mates[0].astype(np.int64), mates[1].astype(np.int64), mates[2].astype(np.int64)
            df['qname_unpaired'] = df['qname']
        if sense is not None:                                       # the frame's index is the row in file order, sorted or not
            df['sense'] = np.array(['+', '-'], dtype=object)[(sense == ord('-')).astype(np.int64)][df.index.values]
        return df

    def _files(self, chrom):
        """The files of one chromosome; stranded: (chrom_coverage {strand: file}, overlap_coverage, read_counts)."""
        cov, ol, counts = super(NativeBamReadsProcessor, self)._files(chrom)
        if self.stranded == 'no':
            return cov, ol, counts
        return {s: cov[:-len('.npz')] + tail + '.npz' for s, tail in zip(STRANDS, ('_plus', '_minus'))}, ol, counts

    def chromosome_coverage_read_counts(self, gene_overlap_dat, chrom_gene_df, chrom_exon_df, chrom):
        """
        BamReadsProcessor's, and for a stranded processor the two passes of include/degnorm_amd.h, "Strand-specific counting":
        chrom_gene_df carries `strand`, '+' or '-' for every gene; each strand's genes get their own overlap structure
        (gene_overlap_dat, the structure of both strands together, is not read) and the rows of their sense.  Written:
        read_counts_<s>_<chr>.csv (all genes, chrom_gene_df order), overlap_coverage_<s>_<chr>.pkl (the overlap genes of '+',
        then of '-') and chrom_coverage_<s>_<chr>_plus.npz / _minus.npz (either is not written when no read reached that
        strand's isolated stage).  When every file the chromosome needs exists, nothing is computed.
        """
        if self.stranded == 'no':
            return super(NativeBamReadsProcessor, self).chromosome_coverage_read_counts(gene_overlap_dat, chrom_gene_df, chrom_exon_df, chrom)
        from pandas import DataFrame
        from scipy import sparse
        from .gene_processing import get_gene_overlap_structure
        if 'strand' not in chrom_gene_df.columns or not chrom_gene_df['strand'].isin(STRANDS).all():
            raise ValueError("a stranded run takes genes with a `strand` column of '+' and '-' "
                             "(GeneAnnotationProcessor(..., strand=True) leaves the other genes out)")
        parts = {}
        for s in STRANDS:
            genes = chrom_gene_df[chrom_gene_df['strand'] == s]
            if len(genes):
                parts[s] = (get_gene_overlap_structure(genes), genes, chrom_exon_df[chrom_exon_df['gene'].isin(genes['gene'])])
        cov_files, ol_cov_file, count_file = self._files(chrom)
        n_ol = sum(len(g) for ov, _, _ in parts.values() for g in ov['overlap_genes'])
        if all(not ov['isolated_genes'] or os.path.isfile(cov_files[s]) for s, (ov, _, _) in parts.items()) \
                and (n_ol == 0 or os.path.isfile(ol_cov_file)) and os.path.isfile(count_file):
            if self.verbose:
                logging.info('SAMPLE {0}, CHR {1} -- all coverage and read count files already present; skipping.'
                             .format(self.sample_id, chrom))
            return None
        chrom_len = int(self.header[self.header.chr == chrom].length.iloc[0])
        anns = {s: Annotation(chrom_len, ov, genes, exons) for s, (ov, genes, exons) in parts.items()}
        rows = self.device_rows(chrom)
        try:
            n_reads = rows.info()[0]
            n_minus = int((rows.fetch_sense() == ord('-')).sum())
            out = {}
            for s, ann in anns.items():
                t0 = time.perf_counter()
                out[s] = rows.coverage(ann, 'device', strand=s)
                self.timing['coverage_s'] = self.timing.get('coverage_s', 0.0) + time.perf_counter() - t0
                self.timing['coverage_device_ms'] = self.timing.get('coverage_device_ms', 0.0) + out[s][5]
                self.timing['pair_device_ms'] = self.timing.get('pair_device_ms', 0.0) + rows.pair_ms
            d = getattr(rows, 'n_dropped', None)
        finally:
            rows.close()
        ol_cov_dict, counts = {}, {}
        for s, ann in anns.items():
            csr, ol, cnt = coverage_outputs(ann, *out[s][:5])
            ol_cov_dict.update(ol)
            counts.update(cnt)
            if csr is not None:
                sparse.save_npz(cov_files[s], matrix=csr)
        if n_ol > 0:
            with open(ol_cov_file, 'wb') as f:
                pkl.dump(ol_cov_dict, f)
        genes = chrom_gene_df['gene'].tolist()
        DataFrame({'gene': genes, self.sample_id: [counts[g] for g in genes]}).to_csv(count_file, index=False)
        if self.verbose:
            note = '' if d is None else '; dropped by flags {flags}, by MAPQ {mapq}, not a mate candidate {not_candidate}'.format(**d)
            logging.info('SAMPLE {0}, CHR {1} -- {2} reads ({3} of sense +, {4} of sense -), {5} counted{6}'.format(
                self.sample_id, chrom, n_reads, n_reads - n_minus, n_minus, sum(counts.values()), note))
        return None

    def _chromosome_coverage(self, chrom, chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df):
        ann = Annotation(chrom_len, gene_overlap_dat, chrom_gene_df, chrom_exon_df)
        rows = self.device_rows(chrom)
        try:
            n_reads = rows.info()[0]
            t0 = time.perf_counter()
            counts, ol_cov, idx, val, n_iso_reads, ms = rows.coverage(ann, self.pair)
            self.timing['coverage_s'] = self.timing.get('coverage_s', 0.0) + time.perf_counter() - t0
            self.timing['coverage_device_ms'] = self.timing.get('coverage_device_ms', 0.0) + ms
            if self.pair == 'device' or rows.by_flag:
                self.timing['pair_device_ms'] = self.timing.get('pair_device_ms', 0.0) + rows.pair_ms
            d = getattr(rows, 'n_dropped', None)
            self._chrom_note = '' if d is None else '; dropped by flags {flags}, by MAPQ {mapq}, not a mate candidate {not_candidate}'.format(**d)
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

    fmt='csi': a .csi index of (min_shift, depth) (include/degnorm_amd.h).  `ioffset` is empty and every reference has
    `loffset`, one offset per entry of `bins` (0 for the pseudo-bin, which is pseudo_bin(depth)); aux: the file's auxiliary
    bytes.  tobytes() gives the inflated bytes of the file, write_index compresses them.
    """

    def __init__(self, refs, n_no_coor=None, fmt='bai', min_shift=14, depth=5, aux=b''):
        self.refs = refs
        self.n_no_coor = n_no_coor
        self.fmt, self.min_shift, self.depth, self.aux = fmt, int(min_shift), int(depth), aux

    @classmethod
    def from_tables(cls, ref_n_bin, ref_n_intv, pseudo, bin_id, bin_n_chunk, chunks, ioffset, n_no_coor, loffset=None, **kw):
        """
        The index of the flat tables dn_bai_fetch fills: per reference its number of bins and of linear-index entries and its
        pseudo-bin's four values; per bin, in reference order, its id and its number of chunks; the (n, 2) chunks and the
        linear-index entries of all of them.  A reference with bins gets its pseudo-bin as the last of them.  loffset: the
        column of dn_csi_loffset, for a .csi index (kw: fmt, min_shift, depth).
        """
        index = cls([], n_no_coor, **kw)
        refs, b, c, w = index.refs, 0, 0, 0
        for r in range(len(ref_n_bin)):
            bins = []
            for k in range(b, b + int(ref_n_bin[r])):
                bins.append((int(bin_id[k]), chunks[c:c + int(bin_n_chunk[k])].copy()))
                c += int(bin_n_chunk[k])
            if bins:
                bins.append((index.pseudo_bin, pseudo[4 * r:4 * r + 4].reshape(2, 2).copy()))
            refs.append({'bins': bins, 'ioffset': ioffset[w:w + int(ref_n_intv[r])].copy()})
            if loffset is not None:
                refs[-1]['loffset'] = [int(x) for x in loffset[b:b + int(ref_n_bin[r])]] + ([0] if bins else [])
            b += int(ref_n_bin[r])
            w += int(ref_n_intv[r])
        return index

    @property
    def pseudo_bin(self):
        return pseudo_bin(self.depth)

    def pseudo(self, tid):
        """(offset of the first record, end of the last, mapped, unmapped) of a reference, or None without a pseudo-bin."""
        for bin_id, ch in self.refs[tid]['bins']:
            if bin_id == self.pseudo_bin:
                return tuple(int(x) for x in ch.reshape(-1)[:4])
        return None

    def tobytes(self):
        if self.fmt == 'csi':
            out = [b'CSI\x01', struct.pack('<iii', self.min_shift, self.depth, len(self.aux)), self.aux, struct.pack('<i', len(self.refs))]
            for ref in self.refs:
                out.append(struct.pack('<i', len(ref['bins'])))
                for (bin_id, ch), loffset in zip(ref['bins'], ref['loffset']):
                    out.append(struct.pack('<IQi', bin_id, loffset, len(ch)))
                    out.append(np.ascontiguousarray(ch, dtype='<u8').tobytes())
            if self.n_no_coor is not None:
                out.append(struct.pack('<Q', self.n_no_coor))
            return b''.join(out)
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


def parse_csi(path):
    """The whole of a .csi index file as a BamIndex: its aux bytes and the order of its bins kept."""
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:2] != b'\x1f\x8b':
        raise ValueError('{0} is not a .csi index'.format(path))
    min_shift, depth, aux, bins, n_no_coor = _csi_fields(path, _csi_bytes(path, raw))
    refs = [{'bins': [(b, ch) for b, _, ch in ref], 'loffset': [lo for _, lo, _ in ref], 'ioffset': np.zeros(0, np.uint64)} for ref in bins]
    return BamIndex(refs, n_no_coor, fmt='csi', min_shift=min_shift, depth=depth, aux=aux)


def _write_replacing(data, path):
    tmp = '{0}.tmp{1}'.format(path, os.getpid())
    try:
        with open(tmp, 'wb') as f:
            f.write(data)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def write_bai(index, path):
    """Write a BamIndex to `path`: to a temporary file next to it, renamed when complete."""
    return _write_replacing(index.tobytes(), path)


def write_index(index, path):
    """
    Write a BamIndex to `path` as its format asks: a .bai as write_bai does, a .csi as BGZF blocks of its bytes (zlib, level
    6) and the end-of-file block; to a temporary file next to it, renamed when complete.
    """
    if index.fmt != 'csi':
        return write_bai(index, path)
    data = index.tobytes()
    blocks = [bgzf_compress(data[k:k + BGZF_BLOCK_DATA], 6) for k in range(0, len(data), BGZF_BLOCK_DATA)]
    return _write_replacing(b''.join(blocks) + BGZF_EOF, path)


def csi_depth(min_shift, longest):
    """The smallest depth with 2^(min_shift + 3 depth) >= longest + 256: this library's rule where the caller names none."""
    depth = 0
    while (1 << (int(min_shift) + 3 * depth)) < int(longest) + 256:
        depth += 1
    return depth


def _index_format(fmt, min_shift, depth):
    """The checked (fmt, min_shift, depth) of build_index's keywords; depth stays None where it is left open."""
    if fmt not in ('bai', 'csi'):
        raise ValueError("fmt must be 'bai' or 'csi', not {0!r}".format(fmt))
    if fmt == 'bai':
        if int(min_shift) != 14 or depth not in (None, 5):
            raise ValueError('a .bai index has min_shift 14 and depth 5; pass fmt=\'csi\' for other values')
        return fmt, 14, 5
    min_shift = int(min_shift)
    if not 1 <= min_shift <= 30:
        raise ValueError('min_shift must be 1 .. 30, not {0}'.format(min_shift))
    if depth is not None and (not 0 <= int(depth) <= 8 or min_shift + 3 * int(depth) > 54):
        raise ValueError('depth must be 0 .. 8 with min_shift + 3 depth at most 54, not {0} (min_shift {1})'.format(depth, min_shift))
    return fmt, min_shift, None if depth is None else int(depth)


class _IndexBuilder(_WindowHandle):
    """
    The index builder of one file (dn_bai_*): on GPU `device`, or (None) the library's host build.  window() takes the file's
    windows in order, finish() closes the pass, fetch() reads the tables out.  ms: the device's milliseconds so far.
    """
    unit = 'dn_bai'

    def __init__(self, path, device, n_ref, segment=0, fmt='bai', min_shift=14, depth=5):
        self.lib, self.path, self.device, self.n_ref, self.h = _lib.load(), path, device, int(n_ref), ctypes.c_void_p()
        self.fmt, self.min_shift, self.depth = fmt, min_shift, depth
        self.ms = {'inflate_device_ms': 0.0, 'frame_device_ms': 0.0, 'index_device_ms': 0.0}
        dev = -1 if device is None else int(device)
        if fmt == 'csi':
            self.call(self.lib.dn_csi_create(dev, self.n_ref, segment, min_shift, depth, ctypes.byref(self.h)), 'dn_csi_create')
        else:
            self.call(self.lib.dn_bai_create(dev, self.n_ref, segment, ctypes.byref(self.h)), 'dn_bai_create')

    def window(self, win):
        """dn_bai_window_host on the window's zlib-inflated data (device=None), dn_bai_window on its blocks as they are."""
        i64, i32 = ctypes.c_int64, ctypes.c_int32
        n_rec = i64(0)
        coffset = np.array([off for off, _ in win.batch], dtype=np.int64)
        if self.device is None:
            data = win.host_data()
            isize = np.array([len(d) for d in data], dtype=np.int32)     # of whole blocks: deflate cannot expand one past int32
            n_data = int(isize.sum(dtype=np.int64))
            joined = np.frombuffer(b''.join(data), dtype=np.uint8) if n_data else np.zeros(1, np.uint8)
            self.call(self.lib.dn_bai_window_host(self.h, _ptr(joined, ctypes.c_uint8), n_data, len(data), _ptr(isize, i32), _ptr(coffset, i64),
                                                  win.head_skip, ctypes.byref(n_rec)), 'dn_bai_window_host')
            return
        args, status = self.window_args(win.blocks, win.verify)
        t = [ctypes.c_double(0.0) for _ in range(3)]
        args += (_ptr(coffset, i64), win.head_skip, _ptr(status, i32), ctypes.byref(n_rec), ctypes.byref(t[0]), ctypes.byref(t[1]),
                 ctypes.byref(t[2]))
        self.call(self.lib.dn_bai_window(self.h, *args), 'dn_bai_window')
        for key, v in zip(('inflate_device_ms', 'frame_device_ms', 'index_device_ms'), t):
            self.ms[key] += float(v.value)
        win.check(status)

    def finish(self, end_voffset):
        """
        dn_bai_finish: end_voffset is the virtual offset of the end of the stream.  Returns its sizes: bins (without pseudo-bins),
        chunks, linear-index entries, records, records without a reference, windows, framing fix-ups.
        """
        sizes = np.zeros(8, dtype=np.int64)
        self.call(self.lib.dn_bai_finish(self.h, int(end_voffset), _ptr(sizes, ctypes.c_int64)), 'dn_bai_finish')
        return sizes

    def fetch(self, sizes):
        """dn_bai_fetch: the finished index (sizes: what finish returned) as a BamIndex."""
        i32, u64 = ctypes.c_int32, ctypes.c_uint64
        n_bins, n_chunks, n_intv = (int(x) for x in sizes[:3])
        ref_n_bin, ref_n_intv = np.zeros(max(self.n_ref, 1), np.int32), np.zeros(max(self.n_ref, 1), np.int32)
        pseudo = np.zeros(max(4 * self.n_ref, 1), np.uint64)
        bin_id, bin_n_chunk = np.zeros(max(n_bins, 1), np.int32), np.zeros(max(n_bins, 1), np.int32)
        chunks, ioffset = np.zeros(max(2 * n_chunks, 1), np.uint64), np.zeros(max(n_intv, 1), np.uint64)
        self.call(self.lib.dn_bai_fetch(self.h, _ptr(ref_n_bin, i32), _ptr(ref_n_intv, i32), _ptr(pseudo, u64), _ptr(bin_id, i32),
                                        _ptr(bin_n_chunk, i32), _ptr(chunks, u64), _ptr(ioffset, u64)), 'dn_bai_fetch')
        loffset = None
        if self.fmt == 'csi':
            loffset = np.zeros(max(n_bins, 1), np.uint64)
            self.call(self.lib.dn_csi_loffset(self.h, _ptr(loffset, u64)), 'dn_csi_loffset')
        return BamIndex.from_tables(ref_n_bin[:self.n_ref], ref_n_intv, pseudo, bin_id, bin_n_chunk,
                                    chunks[:2 * n_chunks].reshape(n_chunks, 2), ioffset, int(sizes[4]), loffset=loffset,
                                    fmt=self.fmt, min_shift=self.min_shift, depth=self.depth)


def build_index(bam_file, device=None, n_jobs=1, window_bytes=256 << 20, segment_bytes=None, stats=None, verify=False, fmt='bai',
                min_shift=14, depth=None):
    """
    The .bai index of a coordinate-sorted BAM file as a BamIndex, from one pass over all its records (csrc/dn_bai.hip; the
    index is defined in include/degnorm_amd.h).  device=k: the blocks of about window_bytes of inflated data go to GPU k as
    they are in the file and are inflated, framed and indexed there; only the tables of run heads and linear-index claims
    come back.  device=None: the blocks are inflated with zlib in n_jobs threads and the library's host build of the same
    source walks them; no GPU is needed.  Both give the same index and the same errors (ValueError naming the file and
    the record).  verify: every block must have the CRC32 of its trailer, checked where the block is inflated (ValueError
    naming the file and the block's offset).  segment_bytes: of the framing (None: the library's default).  stats, a dict, receives
    `inflate_device_ms`, `frame_device_ms`, `index_device_ms`, `frame_fixups`, `records`, `chunks` and `windows`.
    fmt='csi': the .csi index of (min_shift, depth) instead, which holds positions up to 2^(min_shift + 3 depth) where a
    .bai ends at 2^29; depth=None takes csi_depth of the header's longest reference.  Values out of range are a ValueError
    before the file is opened.
    """
    fmt, min_shift, depth = _index_format(fmt, min_shift, depth)
    with _WindowFeed(bam_file, window_bytes, verify, n_jobs if device is None else 1) as feed:
        segment = _segment_arg(segment_bytes)
        _, head_blocks, _, head_skip, refs = feed.header()
        if depth is None:
            depth = csi_depth(min_shift, max([length for _, length in refs] + [0]))
            if depth > 8 or min_shift + 3 * depth > 54:
                raise ValueError('{0}: no .csi index of min_shift {1} holds its longest reference'.format(bam_file, min_shift))
        with _IndexBuilder(bam_file, device, len(refs), segment, fmt, min_shift, depth) as bai:
            end, is_open = None, False                   # the block behind the last one that holds a byte
            # the first window starts inside the block in which the header ends, and holds the bytes behind the header
            for win in feed.whole(head_blocks - 1, -head_skip, head_skip):
                for off, blk in win.batch:
                    if is_open:
                        end = off
                    is_open = _isize(blk) > 0
                bai.window(win)
            if end is None or is_open:
                raise ValueError('{0}: no BGZF end-of-file block; the file is truncated'.format(bam_file))
            sizes = bai.finish(end << 16)
            index = bai.fetch(sizes)
    if stats is not None:
        stats.update(bai.ms, frame_fixups=int(sizes[6]), records=int(sizes[3]), chunks=int(sizes[1]), windows=int(sizes[5]))
    return index


def create_index(bam_file, bai_file=None, overwrite=False, fmt='bai', **kw):
    """
    Build the index of bam_file (build_index's keywords) and write it to bai_file (default bam_file + '.bai', or + '.csi'
    for fmt='csi'); its path.
    """
    _index_format(fmt, kw.get('min_shift', 14), kw.get('depth'))
    bai_file = bam_file + '.' + fmt if bai_file is None else bai_file
    if os.path.exists(bai_file) and not overwrite:
        raise FileExistsError('{0} exists; pass overwrite=True to replace it'.format(bai_file))
    return write_index(build_index(bam_file, fmt=fmt, **kw), bai_file)


def verify_bgzf(path, device=None, n_jobs=1, window_bytes=256 << 20):
    """
    Check a whole BGZF file as `bgzip -t` does: it ends with the end-of-file block, and every block inflates to its ISIZE
    bytes, which have the CRC32 of its trailer.  device=k: the blocks of about window_bytes of inflated data go to GPU k as
    they are in the file, every wavefront inflates and checks one, and only the statuses come back -- no inflated byte is
    written or copied.  device=None: zlib and zlib.crc32 in n_jobs threads.  ValueError names the file and the first bad
    block.  Returns {'blocks', 'compressed_bytes', 'inflated_bytes', 'device_ms'}.
    """
    out = {'blocks': 0, 'compressed_bytes': 0, 'inflated_bytes': 0, 'device_ms': 0.0}
    with _WindowFeed(path, window_bytes, True, n_jobs if device is None else 1) as feed:
        for win in feed.whole():
            blocks = win.blocks
            out['blocks'] += len(blocks)
            out['compressed_bytes'] += sum(len(blk) for blk in blocks)
            out['inflated_bytes'] += sum(_isize(blk) for blk in blocks)
            if device is None:
                win.host_data()
                continue
            args, isize, status = _block_args(blocks)
            out_off, big = _out_offsets(isize, len(blocks))
            if big is not None:
                raise ValueError('{0}: the BGZF block at byte {1} claims an inflated size of {2} bytes'.format(path, win.batch[big][0],
                                                                                                             int(isize[big])))
            ms = ctypes.c_double(0.0)
            args += (_ptr(out_off, ctypes.c_int64), None, _ptr(status, ctypes.c_int32), None, ctypes.byref(ms),
                     _ptr(block_crcs(blocks), ctypes.c_uint32))
            _check(_lib.load().dn_bgzf_inflate_check(int(device), *args), 'dn_bgzf_inflate_check')
            out['device_ms'] += float(ms.value)
            win.check(status)
    return out


def _bin_levels(min_shift, depth):
    """(level, first bin, shift of the bins' span) of the levels below the root."""
    return [(l, ((1 << 3 * l) - 1) // 7, min_shift + 3 * (depth - l)) for l in range(1, depth + 1)]


def reg2bins(beg, end, min_shift=14, depth=5):
    """The bins that may hold records overlapping [beg, end) (SAM specification 5.3; of a .csi index of (min_shift, depth))."""
    beg, end = max(int(beg), 0), min(int(end), 1 << (min_shift + 3 * depth)) - 1
    bins = [0]
    for _, first, shift in _bin_levels(min_shift, depth):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def _csi_low(index, ref, beg):
    """The largest loffset over the stored bins whose interval begins at or before beg: every one bounds the region's records."""
    levels = [(0, 0, index.min_shift + 3 * index.depth)] + _bin_levels(index.min_shift, index.depth)
    low = 0
    for (bin_id, _), loffset in zip(ref['bins'], ref['loffset']):
        if bin_id == index.pseudo_bin:
            continue
        _, first, shift = [lv for lv in levels if lv[1] <= bin_id][-1]
        if (bin_id - first) << shift <= beg:
            low = max(low, int(loffset))
    return low


def index_chunks(index, tid, beg, end):
    """
    The [begin, end) virtual-offset ranges a reader has to scan for the records of reference tid that overlap [beg, end):
    the chunks of reg2bins(beg, end) that end above the linear index's lower bound for beg, sorted and coalesced.  On a .csi
    index the bound is the largest loffset of a stored bin that begins at or before beg.
    """
    ref = index.refs[tid]
    ioffset = ref['ioffset']
    if index.fmt == 'csi':
        low = _csi_low(index, ref, max(int(beg), 0))
        want = set(reg2bins(beg, end, index.min_shift, index.depth))
        want.discard(index.pseudo_bin)
    else:
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


class _Sorter(_WindowHandle):
    """
    The coordinate sort of one file (dn_bam_sort_*): on GPU `device`, or (None) the library's host build.  window() takes the
    file's windows in order and finish() sorts; ends(), read() and deflate() then read the sorted stream out.
    windows and inflate_device_ms: the windows taken and the device's milliseconds of inflate so far.
    """
    unit = 'dn_bam_sort'

    def __init__(self, path, device, n_ref, n_stream, segment, window_bytes):
        self.lib, self.path, self.device, self.window_bytes, self.h = _lib.load(), path, device, window_bytes, ctypes.c_void_p()
        self.windows, self.inflate_device_ms, self.n_bytes, self._lo, self._data = 0, 0.0, 0, 0, b''
        self.call(self.lib.dn_bam_sort_create(-1 if device is None else int(device), int(n_ref), int(n_stream), segment, window_bytes,
                                              ctypes.byref(self.h)), 'dn_bam_sort_create')

    def window(self, win):
        """dn_bam_sort_window_host on the window's zlib-inflated data (device=None), dn_bam_sort_window on its blocks as they are."""
        self.windows += 1
        if self.device is None:
            data = b''.join(win.host_data())
            joined = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
            self.call(self.lib.dn_bam_sort_window_host(self.h, _ptr(joined, ctypes.c_uint8), len(data), win.head_skip), 'dn_bam_sort_window_host')
            return
        args, status = self.window_args(win.blocks, win.verify)
        ms = ctypes.c_double(0.0)
        self.call(self.lib.dn_bam_sort_window(self.h, *(args + (win.head_skip, _ptr(status, ctypes.c_int32), ctypes.byref(ms)))),
                  'dn_bam_sort_window')
        self.inflate_device_ms += float(ms.value)
        win.check(status)

    def finish(self):
        """dn_bam_sort_finish: (records, bytes of the sorted stream, framing fix-ups, device ms of framing, of the sort, of the gather)."""
        n_rec, n_bytes, fix = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        ms = [ctypes.c_double(0.0) for _ in range(3)]
        self.call(self.lib.dn_bam_sort_finish(self.h, ctypes.byref(n_rec), ctypes.byref(n_bytes), ctypes.byref(fix), ctypes.byref(ms[0]),
                                              ctypes.byref(ms[1]), ctypes.byref(ms[2])), 'dn_bam_sort_finish')
        self.n_bytes = int(n_bytes.value)
        return (int(n_rec.value), self.n_bytes, int(fix.value)) + tuple(float(v.value) for v in ms)

    def ends(self, n_records):
        """dn_bam_sort_ends: where the records of the sorted stream end (ascending int64 arrays of at most _ENDS_CHUNK)."""
        for first in range(0, n_records, _ENDS_CHUNK):
            n = min(_ENDS_CHUNK, n_records - first)
            ends = np.zeros(n, np.int64)
            self.call(self.lib.dn_bam_sort_ends(self.h, first, n, _ptr(ends, ctypes.c_int64)), 'dn_bam_sort_ends')
            yield ends

    def read(self, a, b):
        """Bytes [a, b) of the sorted stream; fetched (dn_bam_sort_read) window_bytes at a time, for ranges in ascending order."""
        if b > self._lo + len(self._data):
            n = min(max(self.window_bytes, b - a), self.n_bytes - a)
            arr = np.zeros(max(n, 1), np.uint8)
            self.call(self.lib.dn_bam_sort_read(self.h, a, n, _ptr(arr, ctypes.c_uint8)), 'dn_bam_sort_read')
            self._lo, self._data = a, arr[:n].tobytes()
        return self._data[a - self._lo:b - self._lo]

    def deflate(self, cuts):
        """dn_bam_sort_deflate: the BGZF blocks of the ranges `cuts` of the sorted stream, deflated where the stream lies, and the device ms."""
        i64, i32 = ctypes.c_int64, ctypes.c_int32
        beg = np.array([a for a, _ in cuts] + [0], np.int64)
        lens = np.array([b - a for a, b in cuts] + [0], np.int32)
        cap = int(self.lib.dn_bgzf_deflate_bound(len(cuts), _ptr(lens, i32)))
        out, out_off, ms = np.zeros(max(cap, 1), np.uint8), np.zeros(len(cuts) + 1, np.int64), ctypes.c_double(0.0)
        self.call(self.lib.dn_bam_sort_deflate(self.h, len(cuts), _ptr(beg, i64), _ptr(lens, i32), _ptr(out, ctypes.c_uint8), cap, _ptr(out_off, i64),
                                               ctypes.byref(ms)), 'dn_bam_sort_deflate')
        return memoryview(out)[:int(out_off[len(cuts)])], float(ms.value)


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
    n_jobs = max(int(n_jobs), 1)
    tmp = dst + '.tmp'
    t = {'inflate_device_ms': 0.0, 'deflate_s': 0.0, 'windows': 0, 'deflate_device_ms': 0.0, 'out_bytes': 0}
    try:
        # the pool inflates (device=None) and deflates (deflate='zlib')
        with _WindowFeed(src, window_bytes, verify, n_jobs if device is None or deflate == 'zlib' else 1) as feed:
            segment, window_bytes = _segment_arg(segment_bytes), feed.window_bytes

            def deflated(parts):
                t0 = time.perf_counter()
                one = lambda d: bgzf_compress(d, level)                              # noqa: E731
                out = list(feed.pool.map(one, parts) if feed.pool is not None else map(one, parts))
                t['deflate_s'] += time.perf_counter() - t0
                return out

            # plan memory: the size of the whole stream, and the compressed bytes of the largest window
            data, head_blocks, header_end, head_skip, refs = feed.header()
            _, _, isizes = bgzf_blocks(src)
            n_stream = int(isizes.sum()) - header_end
            if device is not None:
                n_comp_max = 65536 * max(_window_cuts(isizes[head_blocks - 1:].tolist(), window_bytes))
                need = 2 * n_stream + n_comp_max + _SORT_TABLE_BYTES * (n_stream // 128 + 1)
                if deflate == 'native' and n_stream + 64 < _DEFLATE_REGION:      # too small to lend the encoder its slots
                    need += _DEFLATE_REGION
                have = int(DEVICE_MEMORY_SHARE * device_memory(device)[0]) if max_device_bytes is None else int(max_device_bytes)
                if need > have:
                    raise ValueError('{0}: sorting needs about {1} bytes of device memory ({2} bytes of records), {3} are allowed; '
                                     'a file that does not fit the device cannot be sorted here'.format(src, need, n_stream, have))
            with _Sorter(src, device, len(refs), n_stream, segment, window_bytes) as sorter:
                # feed windows: the first starts inside the block in which the header ends, and counts that block whole
                for win in feed.whole(head_blocks - 1, 0, head_skip):
                    sorter.window(win)
                n_rec, n_bytes, fix, frame_ms, sort_ms, gather_ms = sorter.finish()
                t.update(windows=sorter.windows, inflate_device_ms=sorter.inflate_device_ms)
                # write blocks: the header's, then those of the sorted stream, cut where records end
                header = coordinate_header(data[:header_end])
                head_parts = [header[a:a + BGZF_BLOCK_DATA] for a in range(0, len(header), BGZF_BLOCK_DATA)]
                cuts = _block_cuts(sorter.ends(n_rec))
                with open(tmp, 'wb') as f:
                    if deflate == 'native':
                        f.writelines(bgzf_deflate(head_parts))
                        for group in _batched(cuts, window_bytes, weigh=lambda ab: ab[1] - ab[0]):
                            t0 = time.perf_counter()
                            out, ms = sorter.deflate(group)
                            t['deflate_device_ms'] += ms
                            t['deflate_s'] += time.perf_counter() - t0
                            t['out_bytes'] += len(out)
                            f.write(out)
                    else:
                        f.writelines(deflated(head_parts))
                        parts = (sorter.read(a, b) for a, b in cuts)
                        for group in iter(lambda: list(itertools.islice(parts, 64 * n_jobs)), []):
                            for blk in deflated(group):
                                t['out_bytes'] += len(blk)
                                f.write(blk)
                    f.write(BGZF_EOF)
                os.replace(tmp, dst)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    if stats is not None:
        stats.update(t, frame_device_ms=frame_ms, sort_device_ms=sort_ms, gather_device_ms=gather_ms, frame_fixups=fix, records=n_rec,
                     bytes=n_bytes)
    return dst


# --- SAM text -----------------------------------------------------------------------------------------------------------------

SAM_ERRORS = {1: 'empty line', 2: 'fewer than 11 tab-separated fields', 3: 'the read name is empty or longer than 254 bytes',
              4: 'FLAG, POS, MAPQ, PNEXT or TLEN is not a decimal integer in its range',
              5: 'RNAME or RNEXT names a reference the header has no @SQ line for', 6: 'malformed CIGAR',
              7: 'more than 65535 CIGAR operations are not supported', 8: 'empty SEQ field',
              9: "the CIGAR's query length differs from the length of SEQ", 10: 'QUAL is neither * nor as long as SEQ',
              11: "QUAL byte outside '!' .. '~'", 12: 'malformed optional field', 13: 'optional integer out of range',
              14: 'B array value outside the range of its type', 15: 'H field with an odd number of bytes',
              16: 'optional float is not a decimal number'}
SAM_WINDOW_MAX = 1 << 30         # text bytes dn_sam_encode takes at a time


class SamLineError(ValueError):
    """A malformed SAM alignment line: `line` (1-based, within the text that was encoded) and `what`."""

    def __init__(self, line, what):
        ValueError.__init__(self, 'line {0}: {1}'.format(line, what))
        self.line, self.what = line, what


def _fnv1a(name):
    h = 0xcbf29ce484222325
    for c in name:
        h = ((h ^ c) * 0x100000001b3) & 0xffffffffffffffff
    return h


class _SamRefs(object):
    """The reference table dn_sam_encode takes: the names of `refs` ([(name, length)] or names) sorted by their FNV-1a hash."""

    def __init__(self, refs):
        names = [(r if isinstance(r, (str, bytes)) else r[0]) for r in refs]
        names = [n.encode('latin-1') if isinstance(n, str) else bytes(n) for n in names]
        order = sorted(range(len(names)), key=lambda k: (_fnv1a(names[k]), k))
        self.n = len(names)
        self.hash = np.array([_fnv1a(names[k]) for k in order] + [0], np.uint64)
        self.id = np.array(order + [0], np.int32)
        self.len = np.array([len(names[k]) for k in order] + [0], np.int32)
        self.beg = np.zeros(self.n + 1, np.int64)
        np.cumsum(self.len[:self.n], out=self.beg[1:])
        joined = b''.join(names[k] for k in order)
        self.n_names = len(joined)
        self.names = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)

    def args(self):
        c = ctypes
        return (self.n, _ptr(self.hash, c.c_uint64), _ptr(self.id, c.c_int32), _ptr(self.beg, c.c_int64), _ptr(self.len, c.c_int32),
                _ptr(self.names, c.c_uint8), self.n_names)


def _sam_encode(text, table, device, t):
    """dn_sam_encode / dn_sam_encode_host on one window of alignment lines: (record stream as a uint8 array, int64 record offsets).
    t, a dict, gains `lines`, `records`, `float_patches`, `copy_ms` and `encode_device_ms`.  SamLineError for a malformed line."""
    n = len(text)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    if n > SAM_WINDOW_MAX:
        raise ValueError('a window of {0} bytes of SAM text is beyond {1}'.format(n, SAM_WINDOW_MAX))
    a = np.frombuffer(text, dtype=np.uint8)
    lines = text.count(b'\n') + 1
    floats = text.count(b':f:') + (text.count(b',') if b':B:f' in text else 0)
    c, i64 = ctypes, ctypes.c_int64
    out, off, patch = np.zeros(2 * n + 36 * lines, np.uint8), np.zeros(lines + 1, np.int64), np.zeros(2 * floats + 2, np.int64)
    n_lines, n_rec, n_out, n_patch, err_line, err_kind = i64(0), i64(0), i64(0), i64(0), i64(0), c.c_int32(0)
    copy_ms, ms = c.c_double(0.0), c.c_double(0.0)
    args = (_ptr(a, c.c_uint8), n) + table.args() + (_ptr(out, c.c_uint8), out.size, _ptr(off, i64), off.size, _ptr(patch, i64), floats,
                                                     c.byref(n_lines), c.byref(n_rec), c.byref(n_out), c.byref(n_patch), c.byref(err_line),
                                                     c.byref(err_kind))
    lib = _lib.load()
    if device is None:
        _check(lib.dn_sam_encode_host(*args), 'dn_sam_encode_host')
    else:
        _check(lib.dn_sam_encode(int(device), *(args + (c.byref(copy_ms), c.byref(ms)))), 'dn_sam_encode')
    t['lines'] = t.get('lines', 0) + int(n_lines.value)
    t['copy_ms'] = t.get('copy_ms', 0.0) + float(copy_ms.value)
    t['encode_device_ms'] = t.get('encode_device_ms', 0.0) + float(ms.value)
    if err_kind.value:
        raise SamLineError(int(err_line.value), SAM_ERRORS.get(int(err_kind.value), 'error {0}'.format(err_kind.value)))
    t['records'] = t.get('records', 0) + int(n_rec.value)
    t['float_patches'] = t.get('float_patches', 0) + int(n_patch.value)
    return out[:int(n_out.value)], off[:int(n_rec.value) + 1]


def sam_records(text, refs, device=None, stats=None):
    """
    The BAM records of SAM alignment lines: (record stream bytes, int64 offsets at which the records start, one more than
    records: the last is the stream's size).  `text`: bytes of alignment lines, no '@' header lines, the last line with or
    without its '\\n'; `refs`: the @SQ names in header order ([(name, length)] as read_header gives them, or names).  The
    encoding is defined in include/degnorm_amd.h ("SAM text to BAM records"); csrc/dn_sam.hip encodes on GPU `device`, one lane
    per line, or (device=None) its host build does, which needs no GPU; both give the same bytes.  The counterpart of
    frame_records and inflate_blocks.  ValueError 'line <n>: <what>' names the first malformed line (1-based).  stats, a dict,
    receives `lines`, `records`, `float_patches` (float payloads the host filled in with strtod), `copy_ms` and
    `encode_device_ms` (0 on the host).
    """
    t = {}
    try:
        out, off = _sam_encode(bytes(text), _SamRefs(refs), device, t)
    finally:
        if stats is not None:
            stats.update({'lines': 0, 'records': 0, 'float_patches': 0, 'copy_ms': 0.0, 'encode_device_ms': 0.0}, **t)
    return out.tobytes(), off.copy()


def sam_header(f, path):
    """
    Read the '@' header lines off the start of the open SAM file f: (header text as in the file, [(SN, LN)] of its @SQ lines
    in order, number of header lines, the bytes read beyond the header).  ValueError for an @SQ line without SN or LN.
    """
    buf, pos, n_lines, refs, eof = b'', 0, 0, [], False
    while True:
        # the line at pos is whole, or the file at its end, before it is looked at
        while not eof and (pos >= len(buf) or (buf[pos:pos + 1] == b'@' and buf.find(b'\n', pos) < 0)):
            more = f.read(_CHUNK)
            eof = not more
            buf += more
        if buf[pos:pos + 1] != b'@':
            break
        end = buf.find(b'\n', pos)
        end = len(buf) if end < 0 else end + 1
        n_lines += 1
        fields = buf[pos:end].rstrip(b'\r\n').split(b'\t')
        if fields[0] == b'@SQ':
            tags = dict((x[:2], x[3:]) for x in fields[1:] if x[2:3] == b':')
            for tag in (b'SN', b'LN'):
                if tag not in tags:
                    raise ValueError('{0}: line {1}: @SQ line without {2}'.format(path, n_lines, tag.decode()))
            if not tags[b'LN'].isdigit() or int(tags[b'LN']) >= 2 ** 31:
                raise ValueError('{0}: line {1}: @SQ line whose LN is not an integer below 2^31'.format(path, n_lines))
            refs.append((tags[b'SN'].decode('latin-1'), int(tags[b'LN'])))
        pos = end
    return buf[:pos], refs, n_lines, buf[pos:]


def _sam_windows(f, rest, window_bytes):
    """Windows of about window_bytes of the open file f (after `rest`, bytes already read), each cut behind its last '\\n';
    a window without one grows until it has one or the file ends."""
    buf, eof = rest, False
    while True:
        while not eof and (len(buf) < window_bytes or buf.find(b'\n') < 0):
            more = f.read(max(window_bytes - len(buf), 1 << 16))
            eof = not more
            buf += more
        if not buf:
            return
        if eof and len(buf) <= window_bytes:
            cut = len(buf)                            # the end of the file: the last line may lack its '\n'
        else:
            cut = buf.rfind(b'\n', 0, window_bytes) + 1
            if cut == 0:                              # the first line is longer than a window: the window is that line
                cut = buf.find(b'\n') + 1 or len(buf)
        yield buf[:cut]
        buf = buf[cut:]


class _RecordStore(object):
    """The record stream between the encoder and the block writer: windows are appended, ranges read in ascending order."""

    def __init__(self):
        self.lo, self.data = 0, bytearray()

    def append(self, part):
        self.data += part

    def read(self, a, b):
        if a > self.lo:
            del self.data[:a - self.lo]
            self.lo = a
        return bytes(self.data[a - self.lo:b - self.lo])


def sam_to_bam(src, dst, device=None, n_jobs=1, level=1, window_bytes=256 << 20, deflate='zlib', overwrite=False, stats=None):
    """
    Write the SAM file `src` (X.sam, or gzip-compressed X.sam.gz) as the BAM file `dst` (what `samtools view -b` is run for on an aligner's output); returns dst.
    Records keep the order of the lines: nothing is sorted (sort_bam does that).

    The '@' header lines are copied as they are into the BAM header, whose reference list is that of the @SQ lines in order
    (an @SQ line without SN or LN, and a header without @SQ line, are ValueErrors).  The alignment lines go through the
    encoder in windows of about window_bytes (at most 2^30), each cut behind its last line end: on GPU `device`
    (csrc/dn_sam.hip: one lane per line measures its record, a scan places it, one lane per line writes it), or with
    device=None by the host build of the same source, which needs no GPU.  The encoding is defined in
    include/degnorm_amd.h.  Blocks hold at most 0xff00 bytes and end where a record ends (_block_cuts, as in sort_bam); they
    are deflated by zlib at `level` in n_jobs threads, or with deflate='native' by the library's own encoder (bgzf_deflate)
    on the same device (the host build with device=None).  An end-of-file block follows, and dst + '.tmp' becomes dst.
    device=k and device=None write the same file.

    A malformed line is ValueError('<src>: line <n>: <what>') with the 1-based line of the file, the first such line
    winning and the text the same from both builds; neither dst nor dst + '.tmp' is left behind.  FileExistsError when dst
    exists and overwrite is off.  stats, a dict, receives `windows`, `lines` (alignment lines), `records`, `bytes_in` (of
    src), `record_bytes` (the record stream), `bytes_out` (of dst), `float_patches`, `copy_ms`, `encode_device_ms`, `read_s`,
    `encode_s` and `deflate_s`.
    """
    if deflate not in ('zlib', 'native'):
        raise ValueError("deflate must be 'zlib' or 'native', not {0!r}".format(deflate))
    if os.path.exists(dst) and not overwrite:
        raise FileExistsError('{0} exists; pass overwrite=True to replace it'.format(dst))
    n_jobs, window_bytes = max(int(n_jobs), 1), min(max(int(window_bytes), 1), SAM_WINDOW_MAX)
    tmp = dst + '.tmp'
    t = {'windows': 0, 'lines': 0, 'records': 0, 'float_patches': 0, 'copy_ms': 0.0, 'encode_device_ms': 0.0, 'read_s': 0.0,
         'encode_s': 0.0, 'deflate_s': 0.0, 'record_bytes': 0}
    pool = ThreadPoolExecutor(n_jobs) if n_jobs > 1 and deflate == 'zlib' else None

    def deflated(parts, dev):
        t0 = time.perf_counter()
        if deflate == 'native':
            out = bgzf_deflate(parts, dev)
        else:
            one = lambda d: bgzf_compress(d, level)                              # noqa: E731
            out = list(pool.map(one, parts) if pool is not None else map(one, parts))
        t['deflate_s'] += time.perf_counter() - t0
        return out

    try:
        with gz.open_text(src, device=device) as f:            # X.sam.gz: the inflated text, by the same device or the host build
            t0 = time.perf_counter()
            text, refs, n_head, rest = sam_header(f, src)
            t['read_s'] += time.perf_counter() - t0
            if not refs:
                raise ValueError('{0}: no @SQ line in the header'.format(src))
            table, store = _SamRefs(refs), _RecordStore()
            header = b'BAM\x01' + struct.pack('<i', len(text)) + text + struct.pack('<i', len(refs))
            for name, length in refs:
                nm = name.encode('latin-1') + b'\x00'
                header += struct.pack('<i', len(nm)) + nm + struct.pack('<i', length)

            def end_chunks():
                """The record ends of every window, as offsets into the whole stream; the window's records go to the store first."""
                windows = _sam_windows(f, rest, window_bytes)
                while True:
                    t0 = time.perf_counter()
                    win = next(windows, None)
                    t['read_s'] += time.perf_counter() - t0
                    if win is None:
                        return
                    before, t0 = n_head + t['lines'], time.perf_counter()
                    try:
                        rec, off = _sam_encode(win, table, device, t)
                    except SamLineError as e:
                        raise ValueError('{0}: line {1}: {2}'.format(src, before + e.line, e.what))
                    t['encode_s'] += time.perf_counter() - t0
                    t['windows'] += 1
                    store.append(rec.tobytes())
                    base, t['record_bytes'] = t['record_bytes'], t['record_bytes'] + len(rec)
                    yield off[1:] + base

            with open(tmp, 'wb') as out:
                head_parts = [header[a:a + BGZF_BLOCK_DATA] for a in range(0, len(header), BGZF_BLOCK_DATA)]
                out.writelines(deflated(head_parts, None))                   # by the host build, as in sort_bam: one file for every device
                parts = (store.read(a, b) for a, b in _block_cuts(end_chunks()))
                size = 64 * n_jobs if deflate == 'zlib' else 1024
                for group in iter(lambda: list(itertools.islice(parts, size)), []):
                    out.writelines(deflated(group, device))
                out.write(BGZF_EOF)
            t['bytes_in'] = os.path.getsize(src)
        os.replace(tmp, dst)
    finally:
        if pool is not None:
            pool.shutdown()
        if os.path.exists(tmp):
            os.remove(tmp)
    t['bytes_out'] = os.path.getsize(dst)
    if stats is not None:
        stats.update(t)
    return dst
