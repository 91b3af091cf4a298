"""
The library's DEFLATE decoder on the host (dn_bgzf_inflate_host, bam.inflate_blocks(device=None)): the source that also
runs one BGZF block per wavefront on the device, here without a GPU.  Valid streams of every kind must equal zlib byte for
byte; corrupt ones must end in a status, never in a crash, a hang or a write outside the output.
"""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _inflate_cases as ic                                    # noqa: E402
from degnorm_amd import _lib, bam                              # noqa: E402


@pytest.fixture(scope='module')
def cases():
    return ic.valid_cases()


def test_every_valid_case_equals_zlib(cases):
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names) and len(cases) >= 50
    for name, data, payload in cases:
        assert zlib.decompress(payload, -15) == data, name
    got = bam.inflate_blocks(ic.blocks_of(cases))
    for (name, data, _), g in zip(cases, got):
        assert g == data, name
    # one block at a time, between guard bytes
    for name, data, payload in cases:
        rc, status, out = ic.host_inflate(payload, len(data))
        assert (rc, status) == (0, 0) and out == data, name


def test_case_list_covers_what_it_claims(cases):
    by = {n: (d, p) for n, d, p in cases}
    assert by['random-l6'][1][0] & 6 == 0 and len(by['random-l6'][1]) > ic.FULL       # zlib fell back to stored blocks
    assert by['text-fixed'][1][0] & 6 == 2 and by['text-l6'][1][0] & 6 == 4             # fixed and dynamic Huffman
    assert len(by['run-l9'][1]) < 200 and len(by['near-l9'][1]) < 65000 * 0.6          # long runs; matches 32500 bytes back
    assert by['eof'][1] == bam.BGZF_EOF[18:20] and ic.bgzf(by['eof'][1], 0) == bam.BGZF_EOF
    # more than one deflate block in a payload: a flush ends its block and appends an empty stored one
    data, payload, marks = ic.flushed_stream(2)
    assert by['flushes'] == (data, payload) and len(marks) == 2
    for m in marks:
        assert payload[m - 4:m] == ic.SYNC_MARKER and 0 < m < len(payload)
    # counted block by block: flushes put empty stored blocks between dynamic ones, 'joined' holds the blocks of two streams,
    # and zlib starts a new dynamic block every 16 K symbols (a full BGZF block of literals takes four; at levels 6 and 9 the
    # matches keep text and BAM records within one)
    kinds = ic.deflate_block_types(payload)
    assert kinds.count(0) == 2 and len(kinds) >= 5 and kinds[0] != 0 and kinds[-1] != 0
    kinds = ic.deflate_block_types(by['joined'][1])
    assert len(kinds) >= 3 and 0 in kinds[1:-1]
    for name in ('text-huffman', 'bam-huffman', 'text-rle', 'bam-rle'):
        assert len(by[name][0]) == ic.FULL and ic.deflate_block_types(by[name][1]).count(2) >= 2, name
    assert set(ic.deflate_block_types(by['random-l6'][1])) == {0} and ic.deflate_block_types(by['dist-max'][1]) == [0, 1]
    assert ic.deflate_block_types(by['eof'][1]) == [1]
    full = by['text-l9']
    assert len(full[0]) == ic.FULL and bam.inflate_blocks([ic.bgzf(full[1], ic.FULL)]) == [full[0]]
    assert bam.inflate_blocks([]) == [] and bam.inflate_blocks([bam.BGZF_EOF]) == [b'']


def test_hand_made_lone_code_stream():
    kind, payload, isize = ic.crafted()[0]
    assert kind == 'ok-lone' and zlib.decompress(payload, -15) == b'AAAAA'
    assert bam.inflate_blocks([ic.bgzf(payload, isize)]) == [b'AAAAA']


def test_corrupt_input_is_refused_and_never_harms():
    """
    2 165 seeded mutations (bit flips, truncations, wrong ISIZE, broken LEN / NLEN, bad code-length sets, a match before any
    output, trailing bytes).  For each, either zlib accepts the payload as a stream of exactly ISIZE bytes with nothing left
    over, and the decoder returns the same bytes, or the decoder reports a status and inflate_blocks raises ValueError.
    Measured on the host build: zlib accepts 11.8 % of them (255 of 2 165, all of them bit flips that turn one literal or
    one code length into another of the same size), and the decoder accepts exactly those.
    """
    muts = ic.mutations()
    assert len(muts) >= 2000
    kinds = {k for k, _, _ in muts}
    assert {'flip', 'cut', 'isize', 'stored', 'trailing', 'cl-oversubscribed', 'cl-incomplete', 'lit-oversubscribed',
            'lit-incomplete', 'dist-oversubscribed', 'dist-incomplete', 'match-first'} <= kinds
    accepted, seen = 0, set()
    for kind, payload, isize in muts:
        ref = ic.zlib_verdict(payload)
        ok = ref is not None and len(ref) == isize
        rc, status, out = ic.host_inflate(payload, isize)
        assert rc == 0 and 0 <= status <= 7, (kind, rc, status)
        if status == 0:
            assert ok and out == ref, kind
            assert bam.inflate_blocks([ic.bgzf(payload, isize)]) == [ref]
            accepted += 1
        else:
            seen.add(status)
            with pytest.raises(ValueError, match='BGZF block 0 does not inflate'):
                bam.inflate_blocks([ic.bgzf(payload, isize)])
        if kind not in ('flip', 'cut', 'stored'):
            assert status != 0, kind
    print('zlib and the decoder accept {0} of {1} mutations; statuses seen {2}'.format(accepted, len(muts), sorted(seen)))
    assert accepted < 0.2 * len(muts)                           # the test is not vacuous
    assert seen == {1, 2, 3, 4, 5, 6, 7}


def test_decoder_accepts_what_zlib_accepts():
    """Not required of it, but true: no mutation that zlib takes as an exact stream is refused."""
    for kind, payload, isize in ic.mutations():
        ref = ic.zlib_verdict(payload)
        if ref is not None and len(ref) == isize:
            assert ic.host_inflate(payload, isize)[1:] == (0, ref), kind


def test_a_bad_block_names_its_index(cases):
    blocks = ic.blocks_of(cases[:6])
    kind, payload, isize = [m for m in ic.mutations() if m[0] == 'match-first'][0]
    blocks.insert(4, ic.bgzf(payload, isize))
    with pytest.raises(ValueError, match='BGZF block 4 does not inflate: distance too far back'):
        bam.inflate_blocks(blocks)
    with pytest.raises(ValueError, match='65537'):
        bam.inflate_blocks([ic.bgzf(cases[0][2], 65537)])


def test_inconsistent_arrays_are_invalid(cases):
    lib = _lib.load()
    payload = cases[0][2]
    comp = np.frombuffer(payload, np.uint8).copy()
    out, status = np.zeros(2 * 65536 + 8, np.uint8), np.zeros(2, np.int32)
    P, c = ctypes.POINTER, ctypes

    def call(pay_off, pay_len, out_off, n_comp=len(payload)):
        a, b, o = np.array(pay_off, np.int64), np.array(pay_len, np.int32), np.array(out_off, np.int64)
        return lib.dn_bgzf_inflate_host(comp.ctypes.data_as(P(c.c_uint8)), n_comp, len(a), a.ctypes.data_as(P(c.c_int64)),
                                        b.ctypes.data_as(P(c.c_int32)), o.ctypes.data_as(P(c.c_int64)),
                                        out.ctypes.data_as(P(c.c_uint8)), status.ctypes.data_as(P(c.c_int32)))

    n = len(payload)
    assert call([0], [n], [0, len(cases[0][1])]) == _lib.DN_OK and status[0] == 0
    assert call([1], [n], [0, 10]) == _lib.DN_E_INVALID                          # payload runs past comp
    assert b'outside comp' in lib.dn_reads_last_error()
    assert call([-1], [4], [0, 10]) == _lib.DN_E_INVALID
    assert call([0], [-1], [0, 10]) == _lib.DN_E_INVALID
    assert call([n + 1], [0], [0, 10]) == _lib.DN_E_INVALID
    assert call([0], [n], [0, 65537]) == _lib.DN_E_INVALID                       # ISIZE above 65536
    assert call([0], [n], [0, -1]) == _lib.DN_E_INVALID                          # negative ISIZE
    assert call([0, 0], [n, n], [0, 10, 5]) == _lib.DN_E_INVALID                 # out_off not monotone
    assert call([0], [n], [3, 10]) == _lib.DN_E_INVALID                          # out_off does not start at 0
    assert call([0], [n], [0, 10], n_comp=-1) == _lib.DN_E_INVALID
    assert call([0], [n], [0, 65536]) == _lib.DN_OK and status[0] != 0            # a wrong size is the block's own failure


def test_processor_refuses_unknown_inflate_mode(tmp_path):
    import pandas as pd
    import _bam_fixtures as bf
    p = str(tmp_path / 'x.bam')
    bf.write_bam(p, [('c', 10000)], pd.DataFrame({'ref': 0, 'pos': [5, 9], 'qname': ['a', 'b'], 'cigar': ['10M', '10M']}))
    with pytest.raises(ValueError, match='nonsense'):
        bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path), verbose=False, inflate='nonsense')
    for mode in ('host', 'device'):
        assert bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path), verbose=False, inflate=mode).inflate == mode
