"""
GPU tests of the BGZF CRC32 check (csrc/dn_inflate.hip, WaveMem::flush): every valid case verified in one launch, the sizes at
which slicing and flushing change, blocks with wrong bytes (each first judged by the host build of the same source) among
valid ones, the armed windows of the row store, the index builder and the sort handle, the reader on every inflate x frame
combination, build_index, verify_bgzf, sort_bam and the pipeline.  As in test_gpu_inflate.py, corrupt blocks go to the device only
after the valid batch has passed.
"""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _crc_cases as cc                                        # noqa: E402
import _inflate_cases as ic                                    # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_bam import _layout_case, _run, _same             # noqa: E402
from test_gpu_reads import _case                               # noqa: E402
from degnorm_amd import _lib, bam                              # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = []                                             # set by the valid-input test: corrupt blocks run only after it
COMBOS = [('host', 'host'), ('device', 'host'), ('host', 'device'), ('device', 'device')]
KRING = 32768
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 257, KRING - 258 - 1, KRING - 258, KRING - 258 + 1, KRING - 1, KRING, KRING + 1, 65535, 65536)


@pytest.fixture(scope='module')
def cases():
    return ic.valid_cases()


def _edge_blocks():
    """
    (data, block) at the sizes where a slice, a flush or the ring's wrap changes: stored, level 1 and zeros of each.  A stored
    payload of 65 535 bytes or more is longer than the BSIZE field of a block header can say; the readers here take a block's
    length from the bytes they are handed, so such a block gets a header that says 65 536 and is decoded all the same.
    """
    rng = np.random.default_rng(17)
    out = []
    for n in SIZES:
        text = ic._text(rng, n)
        for data, level in ((text, 0), (text, 1), (bytes(n), 6)):
            payload = ic.deflate(data, level)
            blk = ic.bgzf(payload[:60000], n, zlib.crc32(data))
            out.append((data, blk[:16] + struct.pack('<H', min(len(payload) + 25, 0xffff)) + payload + blk[-8:]))
    return out


def test_all_valid_cases_verified_in_one_launch(cases):
    blocks = ic.blocks_of(cases)
    got = bam.inflate_blocks(blocks, device=0, verify=True)
    assert len(got) == len(cases)
    for (name, data, _), g in zip(cases, got):
        assert g == data, name
    order = np.random.default_rng(5).permutation(len(cases))
    got = bam.inflate_blocks([blocks[k] for k in order] * 3, device=0, verify=True)
    for j, g in enumerate(got):
        assert g == cases[order[j % len(cases)]][1], cases[order[j % len(cases)]][0]
    edge = _edge_blocks()
    got = bam.inflate_blocks([b for _, b in edge], device=0, verify=True)
    for k, ((data, _), g) in enumerate(zip(edge, got)):
        assert g == data, (SIZES[k // 3], k % 3)
    _VALID_PASSED.append(True)


def _device_statuses(blocks, with_out=True):
    comp, n_comp, pay_off, pay_len, isize = bam._block_layout(blocks)
    n = len(blocks)
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(isize[:n], out=out_off[1:])
    out, status = np.zeros(int(out_off[-1]) + 1, np.uint8), np.full(n, -9, np.int32)
    crc = bam.block_crcs(blocks)
    P, c = ctypes.POINTER, ctypes
    rc = _lib.load().dn_bgzf_inflate_check(0, comp.ctypes.data_as(P(c.c_uint8)), n_comp, n, pay_off.ctypes.data_as(P(c.c_int64)),
                                           pay_len.ctypes.data_as(P(c.c_int32)), out_off.ctypes.data_as(P(c.c_int64)),
                                           out.ctypes.data_as(P(c.c_uint8)) if with_out else None, status.ctypes.data_as(P(c.c_int32)),
                                           None, None, crc.ctypes.data_as(P(c.c_uint32)))
    assert rc == 0
    return status, [out[out_off[k]:out_off[k + 1]].tobytes() for k in range(n)]


def test_corrupt_blocks_among_valid_ones(cases):
    assert _VALID_PASSED, 'no corrupt block goes to the device before test_all_valid_cases_verified_in_one_launch has passed in this run'
    bad = [blk for _, blk in cc.silent_flips()] + [blk for _, blk, _ in cc.handmade()]
    valid = ic.blocks_of(cases)
    blocks, is_bad = [], []
    for k, blk in enumerate(valid):
        blocks.append(blk)
        is_bad.append(False)
        if k < len(bad):
            blocks.append(bad[k])
            is_bad.append(True)
    assert sum(is_bad) == len(bad) == 4 * cc.PER_CASE + 3
    host, _ = cc.host_statuses(blocks)                          # the host build first: what every block must report
    want = [cc.E_CRC] * (4 * cc.PER_CASE) + [st for _, _, st in cc.handmade()]
    assert host[np.array(is_bad)].tolist() == want and not host[~np.array(is_bad)].any()
    status, data = _device_statuses(blocks)
    assert status.tolist() == host.tolist()
    good = [d for d, b in zip(data, is_bad) if not b]
    assert good == [d for _, d, _ in cases]
    status, _ = _device_statuses(blocks, with_out=False)         # statuses only: nothing written, nothing copied back
    assert status.tolist() == host.tolist()
    with pytest.raises(ValueError, match='BGZF block 1 does not inflate: CRC32 differs from the block trailer'):
        bam.inflate_blocks(blocks[:3], device=0, verify=True)
    assert len(bam.inflate_blocks(blocks[:3], device=0)) == 3    # and without the check the bad block passes, as it always did
    assert bam.inflate_blocks(valid[:8], device=0, verify=True) == [d for _, d, _ in cases[:8]]


def _records(n=900):
    rng = np.random.default_rng(3)
    pos = np.sort(rng.integers(0, 1 << 20, size=n))
    cig = rng.choice(['100M', '40M2000N60M', '5S95M', '50M1I49M', '30M1D70M'], n)
    df = pd.DataFrame({'ref': 0, 'pos': pos, 'qname': ['read.{0}'.format(i) for i in range(n)], 'cigar': cig, 'nh': 1, 'nh_type': 'C'})
    return bf.encode_records(df, 3)


def _blk(data, level):
    return ic.bgzf(ic.deflate(data, level), len(data), zlib.crc32(data))


def test_row_store_windows_armed():
    assert _VALID_PASSED
    rng = np.random.default_rng(23)
    a, z, b = ic._text(rng, ic.FULL), bytes(70000), ic._text(rng, 40000)
    blocks = [_blk(a, 6), _blk(z, 6), _blk(b, 1)]
    head_skip, tail_keep = 1001, 40000 - 777                     # the CRC covers bytes the window never holds
    want = b'carry' + a[head_skip:] + z + b[:tail_keep]
    rows = bam.DeviceRows(0, True, False, device=0)
    try:
        for verify in (False, True, False):
            data, status, _ = rows.inflate(b'carry', blocks, head_skip, tail_keep, verify)
            assert not status.any() and data.tobytes() == want, verify
        # a count that differs from the call's: an error, the arming is spent, the store goes on
        rows.expect_crc(np.zeros(2, np.uint32))
        with pytest.raises(ValueError, match='2 CRC32s were announced .* for 3 blocks'):
            rows.inflate(b'carry', blocks, head_skip, tail_keep)
        data, status, _ = rows.inflate(b'carry', blocks, head_skip, tail_keep)
        assert not status.any() and data.tobytes() == want
        # a call the library refuses for its arguments spends the arming too
        wrong = [blk[:-8] + bytes([blk[-8] ^ 1]) + blk[-7:] for blk in (blocks[0], blocks[2])]
        rows.expect_crc(bam.block_crcs([wrong[0], blocks[1], wrong[1]]))
        with pytest.raises(ValueError, match='dn_bam_rows_inflate: bad argument'):
            rows.inflate(b'carry', blocks, -1, tail_keep)
        data, status, _ = rows.inflate(b'carry', blocks, head_skip, tail_keep)
        assert not status.any() and data.tobytes() == want
        # wrong trailers: caught when armed, and the arming does not reach the call after
        wrong = [blk[:-8] + bytes([blk[-8] ^ 1]) + blk[-7:] for blk in (blocks[0], blocks[2])]
        assert cc.host_statuses(wrong)[0].tolist() == [cc.E_CRC] * 2             # the host build first, as for every bad block
        data, status, _ = rows.inflate(b'', [blocks[0], blocks[1], wrong[1]], 0, -1, True)
        assert status.tolist() == [0, 0, cc.E_CRC]
        data, status, _ = rows.inflate(b'carry', [wrong[0], blocks[1], wrong[1]], head_skip, tail_keep)
        assert not status.any() and data.tobytes() == want
    finally:
        rows.close()

    rec, offs = _records()
    assert len(rec) > 65280 + 70000 + 20000
    cuts = [0, 65280, 65280 + 70000, len(rec)]                   # the middle block inflates to 70 000 bytes
    blocks = [_blk(rec[x:y], 1) for x, y in zip(cuts[:-1], cuts[1:])]
    head_skip, tail_keep = int(offs[3]), (len(rec) - cuts[2]) - 1234
    got = {}
    for verify in (False, True):
        rows = bam.DeviceRows(0, True, False, device=0)
        try:
            status, n_carry, _, _ = rows.inflate_framed(blocks, head_skip, tail_keep, verify)
            assert not status.any()
            got[verify] = (n_carry, rows.info()[:3]) + tuple(x.tobytes() for x in rows.fetch())
            if verify:
                rows.expect_crc(np.zeros(1, np.uint32))
                with pytest.raises(ValueError, match='1 CRC32s were announced'):
                    rows.inflate_framed(blocks, head_skip, tail_keep)
                assert rows.info()[:3] == got[verify][1]
        finally:
            rows.close()
    assert got[True] == got[False] and got[True][1][0] > 500 and got[True][0] > 0


class _Windows(object):
    """dn_bai_* or dn_bam_sort_* through ctypes: one handle that takes windows of whole BGZF blocks, on GPU 0 or (host) the host build."""

    def __init__(self, kind, n_bytes, host=False):
        self.lib, self.kind, self.host, self.h = _lib.load(), kind, host, ctypes.c_void_p()
        if kind == 'bai':
            rc = self.lib.dn_bai_create(-1 if host else 0, 3, 0, ctypes.byref(self.h))
        else:
            rc = self.lib.dn_bam_sort_create(-1 if host else 0, 3, n_bytes, 0, 0, ctypes.byref(self.h))
        assert rc == 0

    def close(self):
        (self.lib.dn_bai_destroy if self.kind == 'bai' else self.lib.dn_bam_sort_destroy)(self.h)

    def expect_crc(self, crc):
        fn = self.lib.dn_bai_expect_crc if self.kind == 'bai' else self.lib.dn_bam_sort_expect_crc
        return fn(self.h, crc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(crc))

    def window(self, blocks, head_skip):
        """(return code, the library's error text, status of every block)."""
        P, c = ctypes.POINTER, ctypes
        comp, n_comp, pay_off, pay_len, isize = bam._block_layout(blocks)
        n, isize32, status = len(blocks), isize.astype(np.int32), np.full(len(blocks), -9, np.int32)
        coffset = np.concatenate([[0], np.cumsum([len(b) for b in blocks])[:-1]]).astype(np.int64)
        if self.host:
            data = np.frombuffer(b''.join(bam.inflate_block(b) for b in blocks), dtype=np.uint8)
            if self.kind == 'bai':
                rc = self.lib.dn_bai_window_host(self.h, data.ctypes.data_as(P(c.c_uint8)), len(data), n, isize32.ctypes.data_as(P(c.c_int32)),
                                                 coffset.ctypes.data_as(P(c.c_int64)), head_skip, ctypes.byref(c.c_int64()))
            else:
                rc = self.lib.dn_bam_sort_window_host(self.h, data.ctypes.data_as(P(c.c_uint8)), len(data), head_skip)
        else:
            args = (self.h, comp.ctypes.data_as(P(c.c_uint8)), n_comp, n, pay_off.ctypes.data_as(P(c.c_int64)),
                    pay_len.ctypes.data_as(P(c.c_int32)), isize32.ctypes.data_as(P(c.c_int32)))
            st = status.ctypes.data_as(P(c.c_int32))
            if self.kind == 'bai':
                rc = self.lib.dn_bai_window(*(args + (coffset.ctypes.data_as(P(c.c_int64)), head_skip, st, ctypes.byref(c.c_int64()), None, None, None)))
            else:
                rc = self.lib.dn_bam_sort_window(*(args + (head_skip, st, None)))
        return rc, self.lib.dn_last_error().decode(), status.tolist()

    def result(self, end_voffset):
        """(return code of the finish call, the index tables or the sorted stream as bytes)."""
        P, c = ctypes.POINTER, ctypes
        if self.kind == 'sort':
            n_rec, n_bytes = c.c_int64(0), c.c_int64(0)
            rc = self.lib.dn_bam_sort_finish(self.h, ctypes.byref(n_rec), ctypes.byref(n_bytes), None, None, None, None)
            if rc != 0:
                return rc, None
            out = np.zeros(n_bytes.value, np.uint8)
            assert self.lib.dn_bam_sort_read(self.h, 0, n_bytes.value, out.ctypes.data_as(P(c.c_uint8))) == 0
            return rc, (n_rec.value, out.tobytes())
        sizes = np.zeros(8, np.int64)
        rc = self.lib.dn_bai_finish(self.h, end_voffset, sizes.ctypes.data_as(P(c.c_int64)))
        if rc != 0:
            return rc, None
        n_bins, n_chunks, n_intv = (int(x) for x in sizes[:3])
        i32 = [np.zeros(max(k, 1), np.int32) for k in (3, 3, n_bins, n_bins)]
        u64 = [np.zeros(max(k, 1), np.uint64) for k in (12, 2 * n_chunks, n_intv)]
        p32, p64 = (lambda a: a.ctypes.data_as(P(c.c_int32))), (lambda a: a.ctypes.data_as(P(c.c_uint64)))
        assert self.lib.dn_bai_fetch(self.h, p32(i32[0]), p32(i32[1]), p64(u64[0]), p32(i32[2]), p32(i32[3]), p64(u64[1]), p64(u64[2])) == 0
        return rc, (sizes[:5].tolist(),) + tuple(a.tobytes() for a in i32 + u64)


@pytest.mark.parametrize('kind', ['bai', 'sort'])
def test_index_and_sort_windows_armed(kind):
    """
    test_row_store_windows_armed's second fixture (_records() cut at 65 280 and 65 280 + 70 000: three blocks, the middle one
    beyond 64 KiB) through the armed windows of the index builder and of the sort handle.  A .bai cannot address a record
    that starts beyond byte 65 535 of its block, so the builder (device and host alike) refuses these blocks' records: for
    'bai' they go through an armed window once, up to that refusal, and the other steps run on the same records cut at
    65 280 and 65 280 + 65 536 and ended at the last record inside the next 65 536 bytes -- three blocks, the middle one of
    the largest size a block can have, 64 KiB.
    """
    assert _VALID_PASSED
    rec, offs = _records()
    head_skip = int(offs[3])
    cuts = [0, 65280, 65280 + 70000, len(rec)]
    if kind == 'bai':
        blocks = [_blk(rec[x:y], 1) for x, y in zip(cuts[:-1], cuts[1:])]
        res = []
        for host in (True, False):
            w = _Windows(kind, 0, host)
            try:
                if not host:
                    assert w.expect_crc(bam.block_crcs(blocks)) == 0
                res.append(w.window(blocks, head_skip))
            finally:
                w.close()
        assert res[1][:2] == res[0][:2] and res[1][0] == _lib.DN_E_INVALID and res[1][2] == [0, 0, 0]
        assert 'starts beyond byte 65535 of its BGZF block' in res[1][1]
        cuts = [0, 65280, 65280 + 65536, int(offs[offs <= 65280 + 2 * 65536][-1])]
    blocks = [_blk(rec[x:y], 1) for x, y in zip(cuts[:-1], cuts[1:])]
    wrong = [blk[:-8] + bytes([blk[-8] ^ 1]) + blk[-7:] for blk in (blocks[0], blocks[2])]
    flipped = [wrong[0], blocks[1], wrong[1]]
    for blk in wrong:                                                             # judged on the host first, as every bad block: by zlib,
        with pytest.raises(bam.BgzfCrcError):                                     # the host build of the decoder stops at 64 KiB
            bam.inflate_block(blk, True)
    n_bytes, end = cuts[-1] - head_skip, sum(len(b) for b in blocks) << 16
    who = 'dn_bai' if kind == 'bai' else 'dn_bam_sort'

    def run(host, steps):
        w = _Windows(kind, n_bytes, host)
        try:
            return steps(w)
        finally:
            w.close()

    want = run(True, lambda w: (w.window(blocks, head_skip)[0], w.result(end)))
    assert want[0] == 0 and want[1][0] == 0 and want[1][1] is not None

    def unarmed(w):
        # a count that differs from the call's: an error with the exact text, the arming is spent, the handle goes on
        assert w.expect_crc(np.zeros(2, np.uint32)) == 0
        rc, text, _ = w.window(blocks, head_skip)
        assert rc == _lib.DN_E_INVALID and text == '{0}_window: 2 CRC32s were announced ({0}_expect_crc) for 3 blocks'.format(who)
        # a call refused for its arguments spends the arming too: the window after it is not checked against these zeros
        assert w.expect_crc(np.zeros(3, np.uint32)) == 0
        rc, text, _ = w.window(blocks, -1)
        assert rc == _lib.DN_E_INVALID and text == who + '_window: bad argument'
        rc, _, status = w.window(blocks, head_skip)
        assert rc == 0 and status == [0, 0, 0]
        return w.result(end)

    def armed(w):
        assert w.expect_crc(bam.block_crcs(blocks)) == 0
        rc, _, status = w.window(blocks, head_skip)
        assert rc == 0 and status == [0, 0, 0]
        return w.result(end)

    def flipped_unarmed(w):                                                       # nobody looks at the trailers
        rc, _, status = w.window(flipped, head_skip)
        assert rc == 0 and status == [0, 0, 0]
        return w.result(end)

    def flipped_armed(w):
        assert w.expect_crc(bam.block_crcs(flipped)) == 0
        rc, _, status = w.window(flipped, head_skip)
        assert rc == 0 and status == [cc.E_CRC, 0, cc.E_CRC]
        rc, text, _ = w.window(blocks, head_skip)                                 # the handle has failed
        assert rc == _lib.DN_E_STATE and text.startswith(who + '_window: ')
        return w.result(end)

    assert run(False, unarmed) == want[1]
    assert run(False, armed) == want[1]
    assert run(False, flipped_unarmed) == want[1]
    assert run(False, flipped_armed) == (_lib.DN_E_STATE, None)


def test_device_sort_verified(damaged, tmp_path):
    """sort_bam(device=0, verify=True): the damaged block is named as the host sort names it; a good file is written as without the check."""
    assert _VALID_PASSED
    path, good_path, chrom, offset = damaged
    dst = str(tmp_path / 'sorted.bam')
    with pytest.raises(ValueError) as host:
        bam.sort_bam(path, dst, device=None, verify=True)
    assert str(host.value) == cc.crc_message(path, offset)
    with pytest.raises(ValueError) as dev:
        bam.sort_bam(path, dst, device=0, verify=True, window_bytes=70000)
    assert str(dev.value) == str(host.value)
    assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')
    got = {}
    for verify in (False, True):
        stats = {}
        with open(bam.sort_bam(good_path, dst, device=0, verify=verify, window_bytes=70000, overwrite=True, stats=stats), 'rb') as f:
            got[verify] = f.read()
        assert stats['windows'] > 1 and stats['records'] > 2000
    assert got[True] == got[False] and len(got[True]) > 10000


@pytest.fixture(scope='module')
def three(tmp_path_factory):
    """test_gpu_inflate's windows case: three references, the middle one's range starts and ends inside shared blocks."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(21, 4000, True)
    df = pd.DataFrame({'ref': 1, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values, 'next_ref': 1})
    before = df.sample(700, random_state=1).assign(ref=0)
    after = df.sample(600, random_state=2).assign(ref=2, qname=lambda d: 'z' + d.qname)
    p = str(tmp_path_factory.mktemp('three') / 'three.bam')
    bf.write_bam(p, [('chrA', chrom_len), (chrom, chrom_len), ('chrZ', chrom_len)], pd.concat([df, before, after]), straddle=True, level=6)
    return p, chrom, ov, gene_df, exon_df


@pytest.mark.parametrize('straddle', [False, True])
@pytest.mark.parametrize('key', ['se', 'qi', 'pe'])
def test_reader_verified_on_goldens(key, straddle, tmp_path):
    """test_gpu_inflate's golden layouts (single-end, query-indexed, paired; records aligned to blocks or straddling them):
    every inflate x frame combination with the check on gives what the host reader gives without it."""
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    if paired:
        pair = z['pe_pair']
        mate = np.zeros(len(pair), dtype=np.int64)
        mate[1:] = (pair[1:] == pair[:-1]).astype(np.int64)
        df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': ['{0}.{1}'.format(a, b + 1) for a, b in zip(pair, mate)],
                           'cigar': reads.cigar.values, 'next_ref': 0})
    else:
        df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': ['r{0}'.format(i) for i in range(len(reads))],
                           'cigar': reads.cigar.values, 'nh': 1, 'nh_type': 'C'})
    p = str(tmp_path / (key + '.bam'))
    bf.write_bam(p, [('c', chrom_len)], df, straddle=straddle, level=1 if key == 'se' else 6)
    proc, want = _run(p, 'c', ov, gene_df, exon_df, tmp_path / 'plain')
    want_frame = proc.load_chromosome_reads('c')
    assert proc.paired == paired and len(want_frame) > 100
    for inflate, frame in COMBOS:
        proc, files = _run(p, 'c', ov, gene_df, exon_df, tmp_path / (inflate + frame), inflate=inflate, frame=frame, verify=True,
                           window_bytes=40000)
        _same(want, files)
        pd.testing.assert_frame_equal(want_frame, proc.load_chromosome_reads('c'))


@pytest.mark.parametrize('window_bytes', [1, 70000])
@pytest.mark.parametrize('inflate,frame', COMBOS)
def test_reader_verified_equals_unverified(inflate, frame, window_bytes, three, tmp_path):
    p, chrom, ov, gene_df, exon_df = three
    res = {}
    for verify in (False, True):
        proc, files = _run(p, chrom, ov, gene_df, exon_df, tmp_path / str(verify), chroms=[chrom], window_bytes=window_bytes,
                           inflate=inflate, frame=frame, verify=verify)
        res[verify] = (files, proc.load_chromosome_reads(chrom))
    _same(res[False][0], res[True][0])
    pd.testing.assert_frame_equal(res[False][1], res[True][1])
    assert len(res[True][1]) > 1000


@pytest.fixture(scope='module')
def damaged(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('crc') / 'd.bam')
    chrom, offset, good = cc.damaged_bam(path)
    good_path = path[:-4] + '_good.bam'
    with open(good_path, 'wb') as f:
        f.write(good)
    return path, good_path, chrom, offset


@pytest.mark.parametrize('inflate,frame', COMBOS)
def test_reader_names_the_damaged_block(inflate, frame, damaged, tmp_path):
    assert _VALID_PASSED
    path, _, chrom, offset = damaged
    kw = dict(output_dir=str(tmp_path / 'o'), verbose=False, inflate=inflate, frame=frame, window_bytes=50000)
    proc = bam.NativeBamReadsProcessor(path, path + '.bai', **kw)
    assert len(proc.load_chromosome_reads(chrom)) > 2000         # unverified: the damaged file loads, as it always did
    proc.verify = True                                           # the constructor's own reads (zlib) are behind it: this is the window path
    with pytest.raises(ValueError) as e:
        proc.load_chromosome_reads(chrom)
    assert str(e.value) == cc.crc_message(path, offset)
    with pytest.raises(ValueError) as e:                         # from the start: whichever read meets the block first names it
        bam.NativeBamReadsProcessor(path, path + '.bai', verify=True, **kw).load_chromosome_reads(chrom)
    assert str(e.value) == cc.crc_message(path, offset)


def test_index_and_file_check_on_the_device(damaged, three):
    assert _VALID_PASSED
    path, good_path, chrom, offset = damaged
    for p in (good_path, three[0]):
        assert bam.build_index(p, device=0, verify=True, window_bytes=70000).tobytes() == bam.build_index(p, device=0, window_bytes=70000).tobytes()
        got, want = bam.verify_bgzf(p, device=0, window_bytes=70000), bam.verify_bgzf(p, device=None)
        assert got.pop('device_ms') > 0 and want.pop('device_ms') == 0 and got == want and got['blocks'] > 3
    bam.build_index(path, device=0)                              # unverified: indexed without a word
    with pytest.raises(ValueError) as e:
        bam.build_index(path, device=0, verify=True, window_bytes=70000)
    assert str(e.value) == cc.crc_message(path, offset)
    with pytest.raises(ValueError) as e:
        bam.verify_bgzf(path, device=0, window_bytes=70000)
    assert str(e.value) == cc.crc_message(path, offset)


def test_pipeline_verified_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, assert_same_table, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.pipeline import run_pipeline
    paths = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.bam'))
        bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1), level=6 if k == 2 else 1)
        paths.append(p)
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    out = str(tmp_path / 'out')
    os.makedirs(out)
    model, estimates, cov, counts_df, genes_df, exon_df, sample_ids = run_pipeline(
        paths, [p + '.bai' for p in paths], GTF, out, degnorm_iter=ITER, nmf_iter=NMF_ITER, minimax_coverage=minimax, verbose=False,
        inflate='device', frame='device', verify=True)
    assert sample_ids == samples
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_cov(cov, cov_e)
    assert all(os.path.isfile(os.path.join(out, name)) for name in RESULT_FILES)
    # the command in a fresh child process, the check on: the same result files
    out_cli = str(tmp_path / 'cli_out')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--verify-crc', '--device-inflate', '--device-frame', '--bam-files'] + paths + \
          ['--bai-files'] + [p + '.bai' for p in paths] + ['-g', GTF, '-o', out_cli, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER),
                                                           '--minimax-coverage', str(minimax)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    for name in RESULT_FILES + ['read_counts.csv']:
        with open(os.path.join(out, name), 'rb') as fa, open(os.path.join(out_cli, name), 'rb') as fb:
            assert fa.read() == fb.read(), name
