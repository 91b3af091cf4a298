"""
The error texts of the C ABI, without a GPU: every call below fails its argument checks before it touches the device, and the
getter of its family (dn_reads_last_error, dn_gtf_last_error, dn_assemble_last_error) must then return the text named here,
with the return code.  The entry points that clear the text on entry leave it empty after a call that succeeds.
"""
import ctypes
import struct

import numpy as np

from degnorm_amd import _lib


def _args(fn, **by_index):
    """One argument per entry of fn.argtypes: None for a pointer, 0 for a number, except the positions given as i<k>=value."""
    args = [None if hasattr(t, 'contents') else 0 for t in fn.argtypes]
    for k, v in by_index.items():
        args[int(k[1:])] = v
    return args


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _frame(buf):
    lib = _lib.load()
    a = np.frombuffer(buf, np.uint8)
    off = np.zeros(4, np.int64)
    n_rec, consumed = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.dn_bam_frame(_ptr(a), a.size, -1, None, _ptr(off), off.size, ctypes.byref(n_rec), ctypes.byref(consumed))
    return rc, int(n_rec.value), int(consumed.value)


def test_read_coverage_bad_argument():
    lib = _lib.load()
    assert lib.dn_read_coverage(*_args(lib.dn_read_coverage, i2=-1)) == _lib.DN_E_INVALID            # n_rows = -1
    assert lib.dn_reads_last_error() == b'dn_read_coverage: bad argument'


def test_reads_cigar_bounds_bad_argument():
    lib = _lib.load()
    assert lib.dn_reads_cigar_bounds(*_args(lib.dn_reads_cigar_bounds, i5=0)) == _lib.DN_E_INVALID   # max_seg = 0
    assert lib.dn_reads_last_error() == b'dn_reads_cigar_bounds: bad argument'


def test_bam_cigar_bounds_bad_op_off():
    lib = _lib.load()
    pos, op_off, ops = np.zeros(2, np.int64), np.array([0, 4, 2], np.int64), np.zeros(4, np.uint32)
    nseg, bounds, end_pos = np.zeros(2, np.int32), np.zeros(4, np.int64), np.zeros(2, np.int64)
    rc = lib.dn_bam_cigar_bounds(0, 2, _ptr(pos), _ptr(op_off), _ptr(ops), 1, _ptr(nseg), _ptr(bounds), _ptr(end_pos))
    assert rc == _lib.DN_E_INVALID
    assert lib.dn_reads_last_error() == b'dn_bam_cigar_bounds: bad op_off'


def test_bam_frame_malformed_record_then_success_clears():
    lib = _lib.load()
    rc, _, _ = _frame(struct.pack('<i', 8) + bytes(8))                          # block_size 8: below the 32 fixed bytes
    assert rc == _lib.DN_E_INVALID
    assert b'malformed BAM record at byte 0' in lib.dn_reads_last_error()
    assert lib.dn_reads_last_error() == b'malformed BAM record at byte 0 of the window (block_size 8)'
    assert _frame(struct.pack('<i', 32) + bytes(32)) == (_lib.DN_OK, 1, 36)
    assert lib.dn_reads_last_error() == b''


def test_gtf_scan_bad_argument():
    lib = _lib.load()
    buf = np.zeros(1, np.uint8)
    assert lib.dn_gtf_scan(*_args(lib.dn_gtf_scan, i1=_ptr(buf), i2=0)) == _lib.DN_E_INVALID         # n_bytes = 0
    assert lib.dn_gtf_last_error() == b'dn_gtf_scan: bad argument'


def test_assemble_coverage_bad_argument():
    lib = _lib.load()
    assert lib.dn_assemble_coverage(*_args(lib.dn_assemble_coverage, i1=100, i2=0, i6=1)) == _lib.DN_E_INVALID    # p = 0
    assert lib.dn_assemble_last_error() == b'dn_assemble_coverage: bad argument'


def _assemble(**change):
    """dn_assemble_coverage on a sound two-sample, two-gene, three-chunk layout with the named arguments replaced; every call of
    the tests below is refused before the device is touched (the output stays as it was)."""
    lib = _lib.load()
    idx, val = np.array([3, 1], np.int32), np.array([5., 7.], np.float32)
    a = dict(nnz=np.array([2, 0], np.int64), indices=(ctypes.c_void_p * 2)(idx.ctypes.data, None),
             values=(ctypes.c_void_p * 2)(val.ctypes.data, None), lengths=np.array([6, 4], np.int64),
             chunk_gene=np.array([0, 0, 1], np.int32), chunk_src=np.array([0, 10, 2], np.int64),
             chunk_dst=np.array([0, 3, 0], np.int64), chunk_len=np.array([3, 3, 4], np.int32))
    a.update(change)
    out = np.full(20, -1.0, np.float32)
    raw = lambda v: v if v is None or not isinstance(v, np.ndarray) else _ptr(v)
    rc = lib.dn_assemble_coverage(0, 100, 2, raw(a['nnz']), a['indices'], a['values'], 2, raw(a['lengths']), 3, raw(a['chunk_gene']),
                                  raw(a['chunk_src']), raw(a['chunk_dst']), raw(a['chunk_len']), _ptr(out), None)
    assert np.all(out == -1.0)
    return rc, lib.dn_assemble_last_error()


ASSEMBLE_REFUSALS = [
    (dict(nnz=None), b'dn_assemble_coverage: null sample table'),
    (dict(indices=None), b'dn_assemble_coverage: null sample table'),
    (dict(values=None), b'dn_assemble_coverage: null sample table'),
    (dict(chunk_gene=None), b'dn_assemble_coverage: null chunk table'),
    (dict(chunk_len=None), b'dn_assemble_coverage: null chunk table'),
    (dict(nnz=np.array([2, -1], np.int64)), b'dn_assemble_coverage: nnz of sample 1 is negative'),
    (dict(nnz=np.array([2, 1], np.int64)), b'dn_assemble_coverage: sample 1 has nnz > 0 and a null index or value array'),
    (dict(indices=(ctypes.c_void_p * 2)(None, None)), b'dn_assemble_coverage: sample 0 has nnz > 0 and a null index or value array'),
    (dict(values=(ctypes.c_void_p * 2)(None, None)), b'dn_assemble_coverage: sample 0 has nnz > 0 and a null index or value array'),
    (dict(lengths=np.array([6, -4], np.int64)), b'dn_assemble_coverage: length of gene 1 is negative'),
    (dict(chunk_gene=np.array([0, 2, 1], np.int32)), b'dn_assemble_coverage: chunk 1 names a gene outside [0, n_genes)'),
    (dict(chunk_gene=np.array([-1, 0, 1], np.int32)), b'dn_assemble_coverage: chunk 0 names a gene outside [0, n_genes)'),
    (dict(chunk_len=np.array([3, 3, -1], np.int32)), b'dn_assemble_coverage: chunk 2 has a negative length'),
    (dict(chunk_dst=np.array([0, -3, 0], np.int64)), b'dn_assemble_coverage: chunk 1 has a negative destination'),
    (dict(chunk_dst=np.array([0, 4, 0], np.int64)), b'dn_assemble_coverage: chunk 1 ends beyond its gene'),
    (dict(chunk_len=np.array([3, 3, 5], np.int32)), b'dn_assemble_coverage: chunk 2 ends beyond its gene'),
    (dict(chunk_dst=np.array([0, 3, 2 ** 62], np.int64), chunk_len=np.array([3, 3, 2 ** 31 - 1], np.int32)),
     b'dn_assemble_coverage: chunk 2 ends beyond its gene'),
    (dict(lengths=np.array([5, 4], np.int64)), b'dn_assemble_coverage: chunk 1 ends beyond its gene'),
]


def test_assemble_coverage_refuses_a_bad_table_before_the_device():
    for change, text in ASSEMBLE_REFUSALS:
        assert _assemble(**change) == (_lib.DN_E_INVALID, text), sorted(change)


def test_inflate_host_payload_outside_comp():
    lib = _lib.load()
    comp, out, status = np.zeros(8, np.uint8), np.zeros(16, np.uint8), np.zeros(1, np.int32)
    pay_off, pay_len, out_off = np.array([1], np.int64), np.array([8], np.int32), np.array([0, 10], np.int64)
    rc = lib.dn_bgzf_inflate_host(_ptr(comp), comp.size, 1, _ptr(pay_off), _ptr(pay_len), _ptr(out_off), _ptr(out), _ptr(status))
    assert rc == _lib.DN_E_INVALID
    assert b'outside comp' in lib.dn_reads_last_error()
    assert lib.dn_reads_last_error() == b'dn_bgzf_inflate_host: payload of block 0 outside comp'
