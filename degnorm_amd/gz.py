"""
gzip-compressed inputs (`*.gtf.gz`, `*.gff3.gz`, `*.sam.gz`): the library's own chunk-parallel inflate, on the host or on a GPU.

    gunzip(src)                 the inflated bytes of every member of a path or a bytes object
    scan(src)                   the guess table and the segment table: what the host and the device build must agree on
    open_text(path)             a binary file-like object (read, close, `with`) over the inflated bytes; for a path that does
                                not end in .gz simply open(path, 'rb')

include/degnorm_amd.h ("gzip streams") defines the format rules, the guess rule, segments, markers and the errors.  A BGZF file
(the first member carries the BC extra subfield: what bgzip writes) is inflated block by block by the BGZF decoder instead
(bam.inflate_blocks).  device=None is the host build and needs no GPU.
"""
import ctypes
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

CHUNK_BYTES = 16 << 10            # of 16, 64 and 256 KiB the fastest on a level-6 GTF (README, "Reading .gz files")
WINDOW_BYTES = 64 << 20
COUNTERS = ('members', 'chunks', 'guessed', 'confirmed', 'jumped', 'fixups', 'segments', 'blocks', 'bytes_in', 'bytes_out')
STAGES = ('copy_ms', 'guess_ms', 'walk_ms', 'windows_ms', 'emit_ms', 'copy_back_ms')
EXIT_BLOCK, EXIT_MEMBER = 0, 1
SUFFIX = '.gz'


def is_gz(path):
    return isinstance(path, str) and path.endswith(SUFFIX)


def strip_gz(path):
    """The path without a final .gz."""
    return path[:-len(SUFFIX)] if is_gz(path) else path


def _source(src):
    """(uint8 array over the compressed bytes -- a read-only map of a file --, name for error messages)"""
    if isinstance(src, str):
        if not os.path.exists(src):
            raise FileNotFoundError('file {0} not found'.format(src))
        if os.path.getsize(src) == 0:
            return np.zeros(0, np.uint8), src
        return np.memmap(src, dtype=np.uint8, mode='r'), src
    return np.frombuffer(src, dtype=np.uint8), '<bytes>'


def is_bgzf(data):
    """True when the first gzip member of `data` (bytes-like) carries BGZF's BC extra subfield."""
    head = bytes(data[:12])
    if len(head) < 12 or head[:3] != b'\x1f\x8b\x08' or not head[3] & 4:
        return False
    xlen = struct.unpack_from('<H', head, 10)[0]
    extra = bytes(data[12:12 + xlen])
    q = 0
    while q + 4 <= len(extra):
        slen = struct.unpack_from('<H', extra, q + 2)[0]
        if extra[q] == 66 and extra[q + 1] == 67 and slen == 2:
            return True
        q += 4 + slen
    return False


class _Stream(object):
    """One dn_gz handle over an array of compressed bytes: pieces() yields the inflated bytes span after span."""

    def __init__(self, comp, name, device, chunk_bytes, window_bytes, verify, emit=True):
        self.lib = _lib.load()
        self.comp, self.name = comp, name                    # the handle reads comp until it is closed
        self.h = ctypes.c_void_p(None)
        rc = self.lib.dn_gz_open(ctypes.c_void_p(comp.ctypes.data if comp.size else None), int(comp.size), -1 if device is None else int(device),
                                 int(CHUNK_BYTES if chunk_bytes is None else chunk_bytes),
                                 int(WINDOW_BYTES if window_bytes is None else window_bytes), int(bool(verify)), int(bool(emit)),
                                 ctypes.byref(self.h))
        _lib._check(rc, 'dn_gz_open')

    def close(self):
        if self.h:
            self.lib.dn_gz_close(self.h)
            self.h = ctypes.c_void_p(None)

    def piece(self):
        """The next span's bytes, or None behind the last one."""
        out, n, done = ctypes.c_void_p(None), ctypes.c_int64(0), ctypes.c_int32(0)
        rc = self.lib.dn_gz_next(self.h, ctypes.byref(out), ctypes.byref(n), ctypes.byref(done))
        try:
            _lib._check(rc, 'dn_gz_next')
        except ValueError as e:
            raise ValueError('{0}: {1}'.format(self.name, e)) from None
        if done.value:
            return None
        return ctypes.string_at(out.value, n.value)

    def stats(self, device):
        c, ms = (ctypes.c_int64 * len(COUNTERS))(), (ctypes.c_double * len(STAGES))()
        _lib._check(self.lib.dn_gz_counters(self.h, c, ms), 'dn_gz_counters')
        d = dict(zip(COUNTERS, (int(v) for v in c)))
        d['bgzf'] = False
        if device is not None:
            d.update(zip(STAGES, (float(v) for v in ms)))
        return d

    def tables(self):
        nc, ns, g, s = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_void_p(None), ctypes.c_void_p(None)
        _lib._check(self.lib.dn_gz_tables(self.h, ctypes.byref(nc), ctypes.byref(g), ctypes.byref(ns), ctypes.byref(s)), 'dn_gz_tables')
        guess = np.frombuffer(ctypes.string_at(g.value, 8 * nc.value), dtype=np.int64) if nc.value else np.zeros(0, np.int64)
        seg = np.frombuffer(ctypes.string_at(s.value, 32 * ns.value), dtype=np.int64) if ns.value else np.zeros(0, np.int64)
        return guess.copy(), seg.reshape(-1, 4).copy()


def _bgzf_pieces(comp, name, device, window_bytes, verify, stats):
    """The data of a BGZF file, a batch of about window_bytes compressed bytes at a time, by the BGZF decoder."""
    from . import bam
    window_bytes = int(WINDOW_BYTES if window_bytes is None else window_bytes)
    buf = memoryview(comp)
    p, n = 0, len(buf)
    stats.update(dict.fromkeys(COUNTERS, 0), bgzf=True, bytes_in=n)
    while p < n:
        batch, size = [], 0
        while p < n and (not batch or size < window_bytes):
            if n - p < 18:
                raise ValueError('{0}: truncated BGZF block at byte {1}'.format(name, p))
            total = bam._block_size(buf, p, name)
            if total is None or total > n - p:
                raise ValueError('{0}: truncated BGZF block at byte {1}'.format(name, p))
            batch.append(buf[p:p + total])
            p += total
            size += total
        data = b''.join(bam.inflate_blocks(batch, device=device, verify=verify))
        stats['members'] += len(batch)
        stats['blocks'] += len(batch)
        stats['bytes_out'] += len(data)
        if data:
            yield data


def _pieces(src, device, chunk_bytes, window_bytes, verify, stats):
    comp, name = _source(src)
    if is_bgzf(comp):
        for data in _bgzf_pieces(comp, name, device, window_bytes, verify, stats):
            yield data
        return
    st = _Stream(comp, name, device, chunk_bytes, window_bytes, verify)
    try:
        while True:
            data = st.piece()
            if data is None:
                break
            yield data
        stats.update(st.stats(device))
    finally:
        st.close()


def gunzip(src, device=None, chunk_bytes=None, window_bytes=None, verify=True, stats=None):
    """
    The inflated bytes of all members of `src` (a path or bytes).  device=None: the host build, no GPU needed; a device index:
    the kernels.  chunk_bytes (a power of two, default 16 KiB) is the grid the compressed bytes are guessed on, window_bytes
    (default 64 MiB) about how many compressed bytes are on the device at a time: neither changes the bytes or the errors.
    verify: compare every member's CRC32 (its ISIZE always is).  Malformed input raises ValueError('<file>: gzip member at byte
    <offset>: <what>').  stats (dict) receives the counters COUNTERS, `bgzf`, and on a device the stage times STAGES (HIP events).
    """
    stats = {} if stats is None else stats
    return b''.join(_pieces(src, device, chunk_bytes, window_bytes, verify, stats))


def scan(src, device=None, chunk_bytes=None, stats=None):
    """
    The tables of a gzip file taken as one span: (guess, segments) -- guess[c] the guessed entry bit of chunk c or -1, int64;
    segments an (n, 4) int64 array of entry bit, exit bit, output length and exit kind (EXIT_BLOCK, EXIT_MEMBER) in chain order.
    Nothing is decoded for real: CRC32s are not compared, distances are not checked.  stats as gunzip.
    """
    comp, name = _source(src)
    st = _Stream(comp, name, device, chunk_bytes, 1 << 30, False, emit=False)
    try:
        while st.piece() is not None:
            pass
        if stats is not None:
            stats.update(st.stats(device))
        return st.tables()
    finally:
        st.close()


def inflated_size(src, device=None, chunk_bytes=None):
    """The number of bytes `src` inflates to, from a scan (the sum of the segments' output lengths), not from ISIZE."""
    comp, _ = _source(src)
    if is_bgzf(comp):
        return sum(len(d) for d in _pieces(src, device, chunk_bytes, None, False, {}))
    return int(scan(src, device, chunk_bytes)[1][:, 2].sum())


class _Ahead(object):
    """The pieces of an iterator, each asked for on one worker thread while the caller still uses the one before it: the next
    span is inflating (the library call releases the interpreter) while the last one is being read.  An error of a piece is
    raised where that piece would have been returned."""

    def __init__(self, it):
        self._it = it
        self._pool = ThreadPoolExecutor(1)
        self._next = self._pool.submit(next, it, None)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next is None:
            raise StopIteration
        data = self._next.result()
        self._next = self._pool.submit(next, self._it, None) if data is not None else None
        if data is None:
            raise StopIteration
        return data

    def close(self):
        if self._next is not None:
            try:
                self._next.result()              # the worker is inside the library: let it come back before the handle closes
            except Exception:
                pass
            self._next = None
        self._pool.shutdown()
        self._it.close()


class GzReader(object):
    """read(n) / close() over the inflated bytes of a .gz file, a span at a time and one span ahead."""

    def __init__(self, path, device=None, chunk_bytes=None, window_bytes=None, verify=True):
        self.name = path
        self.stats = {}
        self._it = _Ahead(_pieces(path, device, chunk_bytes, window_bytes, verify, self.stats))
        self._buf, self._at = b'', 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._it is not None:
            self._it.close()
            self._it = None
        self._buf, self._at = b'', 0

    def read(self, n=-1):
        if n is None or n < 0:
            rest = [self._buf[self._at:]] + (list(self._it) if self._it is not None else [])
            self._buf, self._at = b'', 0
            return b''.join(rest)
        parts, need = [], n
        while need > 0:
            if self._at >= len(self._buf):
                self._buf, self._at = (next(self._it, b'') if self._it is not None else b''), 0
                if not self._buf:
                    break
            take = self._buf[self._at:self._at + need]
            self._at += len(take)
            need -= len(take)
            parts.append(take)
        return parts[0] if len(parts) == 1 else b''.join(parts)


def open_text(path, device=None, chunk_bytes=None, window_bytes=None, verify=True):
    """A binary reader of the text in `path`: the file itself, or for a path that ends in .gz its inflated bytes."""
    if not is_gz(path):
        return open(path, 'rb')
    return GzReader(path, device, chunk_bytes, window_bytes, verify)
