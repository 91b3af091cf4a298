"""
Host tests of the BGZF CRC32 check (no GPU): the slice-and-combine CRC of csrc/dn_inflate.hip against zlib.crc32, no false
positive on any valid case, blocks that every decoder accepts with wrong bytes (found with zlib) refused once verify is on,
and a BAM file with one changed byte through the reader, the index builder and verify_bgzf.
"""
import ctypes
import os
import shutil
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _crc_cases as cc                                        # noqa: E402
import _inflate_cases as ic                                    # noqa: E402
from degnorm_amd import _lib, bam                              # noqa: E402

LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 32767, 32768, 32769, 65535, 65536, 70001)


def _crc32_host(data, lanes, flush_bytes):
    a = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    crc = ctypes.c_uint32(0xdeadbeef)
    rc = _lib.load().dn_bgzf_crc32_host(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(data), lanes, flush_bytes, ctypes.byref(crc))
    return rc, crc.value


@pytest.mark.parametrize('fill', ['random', 'zeros', 'ones'])
def test_sliced_crc_equals_zlib(fill):
    rng = np.random.default_rng(11)
    for n in LENGTHS:
        data = {'random': bytes(rng.integers(0, 256, size=n, dtype=np.uint8)), 'zeros': bytes(n), 'ones': b'\xff' * n}[fill]
        want = zlib.crc32(data)
        for lanes in (1, 2, 3, 63, 64):
            for flush_bytes in (64, 4096, 32768):
                assert _crc32_host(data, lanes, flush_bytes) == (0, want), (n, lanes, flush_bytes)


def test_sliced_crc_refuses_bad_lane_counts():
    for lanes in (0, 65, -1):
        rc, _ = _crc32_host(b'abc', lanes, 64)
        assert rc == _lib.DN_E_INVALID
        assert 'lanes' in _lib.load().dn_last_error().decode()
    assert _crc32_host(b'abc', 64, 0)[0] == _lib.DN_E_INVALID
    assert _crc32_host(b'abc', 64, 1) == (0, zlib.crc32(b'abc'))


def test_no_false_positives_on_valid_cases():
    cases = ic.valid_cases()
    names = [name for name, _, _ in cases]
    assert {'eof', 'dist-max', 'flushes', 'joined', 'text-l0', 'text-fixed', 'bam-l6'} <= set(names)
    blocks = ic.blocks_of(cases)
    plain = bam.inflate_blocks(blocks)
    checked = bam.inflate_blocks(blocks, verify=True)
    for (name, data, _), a, b, blk in zip(cases, plain, checked, blocks):
        assert a == data and b == data, name
        assert bam.inflate_block(blk, verify=True) == data, name
    status, _ = cc.host_statuses(blocks)
    assert not status.any()


def test_silent_corruption_is_caught():
    flips = cc.silent_flips()
    assert len(flips) == 4 * cc.PER_CASE
    for name, blk in flips:
        # today's behaviour: the block passes every check there was
        assert len(bam.inflate_blocks([blk])[0]) == len(bam.inflate_block(blk)) == int.from_bytes(blk[-4:], 'little'), name
        with pytest.raises(ValueError, match='CRC32 differs from the block trailer'):
            bam.inflate_blocks([blk], verify=True)
        with pytest.raises(ValueError, match='CRC32'):
            bam.inflate_block(blk, verify=True)
    status, _ = cc.host_statuses([blk for _, blk in flips])
    assert (status == cc.E_CRC).all()
    status, _ = cc.host_statuses([blk for _, blk in flips], verify=False)
    assert not status.any()


def test_handmade_cases_and_decode_errors_win():
    made = cc.handmade()
    valid = ic.blocks_of(ic.valid_cases()[:3])
    blocks = [valid[0]] + [blk for _, blk, _ in made] + [valid[1]]
    status, data = cc.host_statuses(blocks)
    assert status.tolist() == [0] + [st for _, _, st in made] + [0]
    assert made[2][2] not in (0, cc.E_CRC)                      # the block that does not decode keeps its decode error
    assert data[0] == ic.valid_cases()[0][1]
    for name, blk, st in made[:2]:
        bam.inflate_blocks([blk])                                # accepted without the check
        with pytest.raises(ValueError, match='BGZF block 1 does not inflate: CRC32 differs from the block trailer'):
            bam.inflate_blocks([valid[2], blk], verify=True)
    with pytest.raises(ValueError, match='does not inflate: ' + bam.INFLATE_ERRORS[made[2][2]]):
        bam.inflate_blocks([made[2][1]], verify=True)
    assert bam.INFLATE_ERRORS[8] == 'CRC32 differs from the block trailer'


def test_checked_inflate_may_drop_the_bytes():
    """out == NULL: statuses only (what verify_bgzf uses on the device), here on the host build."""
    blocks = ic.blocks_of(ic.valid_cases()[:6]) + [cc.handmade()[0][1]]
    comp, n_comp, pay_off, pay_len, isize = bam._block_layout(blocks)
    n = len(blocks)
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(isize[:n], out=out_off[1:])
    status, crc = np.full(n, -9, np.int32), bam.block_crcs(blocks)
    P, c = ctypes.POINTER, ctypes
    args = (comp.ctypes.data_as(P(c.c_uint8)), n_comp, n, pay_off.ctypes.data_as(P(c.c_int64)), pay_len.ctypes.data_as(P(c.c_int32)),
            out_off.ctypes.data_as(P(c.c_int64)), None, status.ctypes.data_as(P(c.c_int32)))
    assert _lib.load().dn_bgzf_inflate_check_host(*(args + (crc.ctypes.data_as(P(c.c_uint32)),))) == 0
    assert status.tolist() == [0] * 6 + [cc.E_CRC]
    assert _lib.load().dn_bgzf_inflate_host(*args) == _lib.DN_E_INVALID        # the old entry point still wants its out


@pytest.fixture(scope='module')
def damaged(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('crc') / 'd.bam')
    chrom, offset, good = cc.damaged_bam(path)
    good_path = path[:-4] + '_good.bam'
    with open(good_path, 'wb') as f:
        f.write(good)
    shutil.copy(path + '.bai', good_path + '.bai')                # one byte differs: the same index serves both
    return path, good_path, chrom, offset


def _read_all(path, chrom, verify, **kw):
    proc = bam.NativeBamReadsProcessor(path, path + '.bai', verbose=False, verify=verify, **kw)
    data = b''.join(proc.windows(chrom))
    off, used, _ = bam.frame_records(data, 0)
    assert used == len(data)
    return data, off


def test_damaged_file_reader(damaged):
    path, good_path, chrom, offset = damaged
    data, off = _read_all(path, chrom, False)                    # today's behaviour: the damaged file frames and loads
    want, want_off = _read_all(good_path, chrom, False)
    assert len(data) == len(want) and data != want and off.tolist() == want_off.tolist() and len(off) == 3000
    for kw in ({}, {'n_jobs': 3}, {'window_bytes': 30000}):
        with pytest.raises(ValueError) as e:
            _read_all(path, chrom, True, **kw)
        assert str(e.value) == cc.crc_message(path, offset)
    assert _read_all(good_path, chrom, True)[0] == want


def test_damaged_file_index_and_file_check(damaged):
    path, good_path, chrom, offset = damaged
    plain = bam.build_index(path)                                # today's behaviour: indexed without a word
    for n_jobs in (1, 3):
        with pytest.raises(ValueError) as e:
            bam.build_index(path, device=None, n_jobs=n_jobs, verify=True)
        assert str(e.value) == cc.crc_message(path, offset)
        with pytest.raises(ValueError) as e:
            bam.verify_bgzf(path, device=None, n_jobs=n_jobs, window_bytes=50000)
        assert str(e.value) == cc.crc_message(path, offset)
    assert bam.build_index(good_path, verify=True).tobytes() == plain.tobytes()
    offs, sizes, isizes = bam.bgzf_blocks(good_path)
    got = bam.verify_bgzf(good_path, device=None, n_jobs=2, window_bytes=50000)
    assert got == {'blocks': len(offs), 'compressed_bytes': int(sizes.sum()), 'inflated_bytes': int(isizes.sum()), 'device_ms': 0.0}
    with open(good_path, 'rb') as f:
        cut = f.read()[:-len(bam.BGZF_EOF)]
    short = good_path[:-4] + '_cut.bam'
    with open(short, 'wb') as f:
        f.write(cut)
    with pytest.raises(ValueError, match='no BGZF end-of-file block'):
        bam.verify_bgzf(short)


def test_header_block_is_checked_too(damaged, tmp_path):
    path, good_path, chrom, offset = damaged
    with open(good_path, 'rb') as f:
        raw = bytearray(f.read())
    at = raw.index(b'SO:coordinate')                             # the header text, verbatim in the first (stored) block
    raw[at + 3] = ord('C')
    p = str(tmp_path / 'h.bam')
    with open(p, 'wb') as f:
        f.write(bytes(raw))
    assert bam.read_header(p) == bam.read_header(good_path)
    with pytest.raises(ValueError) as e:
        bam.read_header(p, verify=True)
    assert str(e.value) == cc.crc_message(p, 0)
    with pytest.raises(ValueError) as e:
        bam.build_index(p, verify=True)
    assert str(e.value) == cc.crc_message(p, 0)


def test_host_pool_names_a_block_beyond_64k(tmp_path):
    """zlib accepts a block that inflates to more than 65 536 bytes, the library's one-shot decoder does not: with the check
    on, the zlib pool itself names such a block, with the agreed text."""
    big = bytes(70000)
    good = ic.bgzf(ic.deflate(big, 6), len(big), zlib.crc32(big))
    bad = ic.bgzf(ic.deflate(big, 6), len(big), zlib.crc32(big) ^ 4)
    for pool_jobs in (None, 2):
        pool = None if pool_jobs is None else bam.ThreadPoolExecutor(max_workers=pool_jobs)
        try:
            assert bam._host_inflate('f.bam', [(0, good), (500, bad)], pool) == [big, big]
            assert bam._host_inflate('f.bam', [(0, good), (500, good)], pool, True) == [big, big]
            with pytest.raises(ValueError) as e:
                bam._host_inflate('f.bam', [(0, good), (500, bad), (900, bad)], pool, True)
            assert str(e.value) == cc.crc_message('f.bam', 500)
        finally:
            if pool is not None:
                pool.shutdown()


def test_arming_a_host_index_builder_is_a_state_error():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.dn_bai_create(-1, 1, 0, ctypes.byref(h)) == 0
    try:
        crc = np.zeros(2, np.uint32)
        assert lib.dn_bai_expect_crc(h, crc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 2) == _lib.DN_E_STATE
        assert lib.dn_bai_expect_crc(None, None, 0) == _lib.DN_E_INVALID
    finally:
        lib.dn_bai_destroy(h)


def test_new_symbols_are_declared_and_bound():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    syms = ge.header_symbols()
    lib = _lib.load()
    for s in ('dn_bgzf_crc32_host', 'dn_bgzf_inflate_check_host', 'dn_bgzf_inflate_check', 'dn_bam_rows_expect_crc', 'dn_bai_expect_crc'):
        assert s in syms and getattr(lib, s).argtypes
    with open(os.path.join(ROOT, 'include', 'degnorm_amd.h')) as f:
        assert '#define DN_INFLATE_E_CRC       8' in f.read()
