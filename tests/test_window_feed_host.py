"""
Host tests of the BGZF window feed of degnorm_amd.bam (no GPU): the cut rule of the whole-file windows against a plain loop
over the file's ISIZEs, for both starting counts, and the window counts build_index and sort_bam report; the trimmed windows
of a reference's index range against the bytes its records occupy in the inflated file; and the text of a block that does
not inflate, which the reader's host inflate shares with the index builder.
"""
import os
import struct
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _inflate_cases as ic                                    # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

REFS = [('c1', 200000), ('c2', 100000)]


def _reads(n, seed=0):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({'ref': rng.choice([0, 1], n), 'pos': rng.integers(0, 90000, n), 'qname': ['r{0}'.format(i) for i in range(n)],
                         'cigar': rng.choice(['50M', '20M100N30M', '5S40M5S', '10M2I10M1D18M'], n)})


@pytest.fixture(scope='module')
def two_refs(tmp_path_factory):
    """Two references in blocks of 20 000 bytes that records straddle: the second one's range starts and ends inside blocks."""
    p = str(tmp_path_factory.mktemp('feed') / 't.bam')
    bf.write_bam(p, REFS, _reads(3000), straddle=True, block_size=20000)
    return p


def _rule(isizes, first, window_bytes, size0):
    """The cut rule, written out: the block ordinals of each window from block `first` on."""
    wins, cur, size = [], [], size0
    for k in range(first, len(isizes)):
        cur, size = cur + [k], size + int(isizes[k])
        if size >= window_bytes:
            wins, cur, size = wins + [cur], [], 0
    return wins + [cur] if cur else wins


@pytest.mark.parametrize('window_bytes', [1, 70000, None])
def test_whole_file_windows_follow_the_cut_rule(two_refs, window_bytes, tmp_path):
    offs, _, isizes = bam.bgzf_blocks(two_refs)
    w = 256 << 20 if window_bytes is None else window_bytes
    with bam._WindowFeed(two_refs, window_bytes) as feed:
        assert feed.window_bytes == w
        _, head_blocks, _, head_skip, refs = feed.header()
        assert refs == REFS and head_skip > 0 and len(offs) - head_blocks >= 6
        want = {}
        for size0 in (-head_skip, 0):                            # build_index leaves the header's bytes out, sort_bam counts the block whole
            want[size0] = _rule(isizes, head_blocks - 1, w, size0)
            wins = list(feed.whole(head_blocks - 1, size0, head_skip))
            got = [[off for off, _ in win.batch] for win in feed.whole(head_blocks - 1, size0, head_skip)]
            assert got == [[int(offs[k]) for k in ks] for ks in want[size0]]
            assert [win.head_skip for win in wins] == [head_skip] + [0] * (len(wins) - 1) and all(win.tail_keep == -1 for win in wins)
            assert all(win.batch is None for win in wins)        # no window keeps its blocks once the next one is read
    if window_bytes == 1:                                        # a window per block; the header's block has no byte of its own to count
        assert len(want[0]) == len(offs) - head_blocks + 1 and len(want[-head_skip]) == len(want[0]) - 1
    elif window_bytes is None:
        assert len(want[0]) == len(want[-head_skip]) == 1
    else:
        assert 2 < len(want[0]) < len(offs) - head_blocks and max(len(ks) for ks in want[0]) > 1
    stats = {}
    bam.build_index(two_refs, device=None, window_bytes=window_bytes, stats=stats)
    assert stats['windows'] == len(want[-head_skip])
    stats = {}
    bam.sort_bam(two_refs, str(tmp_path / 'sorted.bam'), device=None, window_bytes=window_bytes, stats=stats)
    assert stats['windows'] == len(want[0])


def test_starting_counts_can_cut_differently():
    """A first block of 100 bytes of which 60 are the header's: it fills a window of 100 bytes only when it counts whole."""
    assert list(bam._window_cuts([100, 50, 50, 10], 100, 0)) == [1, 2, 1]
    assert list(bam._window_cuts([100, 50, 50, 10], 100, -60)) == [3, 1]
    assert list(bam._window_cuts([], 100)) == [] and list(bam._window_cuts([0, 0], 1)) == [2]


@pytest.mark.parametrize('window_bytes', [1, None])
def test_range_windows_hold_the_records_of_the_reference(two_refs, window_bytes):
    data = b''.join(bam.inflate_block(blk) for _, blk in bam.iter_blocks(two_refs))
    rec = data[bam.parse_header(data)[0]:]
    off, used, _ = bam.frame_records(rec)
    assert used == len(rec)
    tid = np.array([struct.unpack_from('<i', rec, int(o) + 4)[0] for o in off])
    ends = np.append(off[1:], len(rec))
    index = bam.read_bai(two_refs + '.bai')[0]
    with bam._WindowFeed(two_refs, window_bytes) as feed:
        for ref in (0, 1):
            mine = np.flatnonzero(tid == ref)
            assert len(mine) > 1000 and (np.diff(mine) == 1).all()
            wins = [(win.head_skip, win.tail_keep, win.host_bytes()) for win in feed.reference(bam.reference_range(index[ref]))]
            assert b''.join(w[2] for w in wins) == rec[int(off[mine[0]]):int(ends[mine[-1]])]
            assert all(w[0] == 0 for w in wins[1:]) and all(w[1] == -1 for w in wins[:-1])
            assert len(wins) == 1 if window_bytes is None else len(wins) > 3
            if ref == 1:
                assert wins[0][0] > 0                            # the range starts inside a block it shares with c1
            else:
                assert wins[-1][1] > 0                           # and c1's ends inside that block
        assert list(feed.reference(None)) == []


def test_reader_names_a_block_that_does_not_inflate_as_the_index_builder_does(tmp_path):
    """With inflate='host' the reader inflates through _host_inflate: the file, the block's offset and the decoder's words."""
    p = str(tmp_path / 'd.bam')
    bf.write_bam(p, REFS, _reads(3000, seed=1), block_size=20000, level=6)      # c1 stays clean: the constructor reads its first records
    offs, sizes, _ = bam.bgzf_blocks(p)
    vbeg, vend = bam.reference_range(bam.read_bai(p + '.bai')[0][1])
    inside = [k for k in range(len(offs)) if (vbeg >> 16) < offs[k] < (vend >> 16)]
    k = inside[len(inside) // 2]
    raw = bytearray(open(p, 'rb').read())
    blk = bytes(raw[offs[k]:offs[k] + sizes[k]])
    isize = int.from_bytes(blk[-4:], 'little')
    hit = None
    for byte in range(18, 18 + 40):                              # a header byte whose flip neither the host build nor zlib accepts
        q = bytearray(blk)
        q[byte] ^= 0x10
        status = ic.host_inflate(bytes(q[18:-8]), isize)[1]
        if status != 0 and ic.zlib_verdict(bytes(q[18:-8])) is None:
            hit = byte
            break
    assert hit is not None
    raw[offs[k] + hit] ^= 0x10
    with open(p, 'wb') as f:
        f.write(bytes(raw))
    with pytest.raises(ValueError) as e:
        bam.build_index(p, device=None)
    expect = str(e.value)
    assert expect == bam._block_error(p, int(offs[k]), status)
    for kw in ({}, {'n_jobs': 3}, {'window_bytes': 30000}):
        proc = bam.NativeBamReadsProcessor(p, p + '.bai', verbose=False, **kw)
        with pytest.raises(ValueError) as e:
            b''.join(proc.windows('c2'))
        assert str(e.value) == expect and type(e.value) is ValueError
        assert len(b''.join(proc.windows('c1'))) > 0             # the other reference still reads
