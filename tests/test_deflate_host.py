"""
Host tests (no GPU) of the library's DEFLATE encoder, the host build of csrc/dn_deflate.hip: degnorm_amd.bam.bgzf_deflate on
the inputs of tests/_deflate_cases.py, judged by zlib, by the library's own decoder and by verify_bgzf; the size conditions
that show that the matcher and the coder work; the code-length builder on its own (dn_deflate_code_lengths_host); and
sort_bam(deflate='native') on the cases of tests/_sort_cases.py.

The index of a 'native' file is compared with the index of the 'zlib' file of the same case after both have had their virtual
offsets resolved to offsets in the inflated file (_deflate_cases.resolved): the two files hold the same blocks' data, but
their blocks' compressed sizes, and so the compressed half of every virtual offset, differ.
"""
import argparse
import ctypes
import heapq
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _deflate_cases as dc                                    # noqa: E402
import _sort_cases as sc                                       # noqa: E402
from degnorm_amd import _lib, bam                              # noqa: E402

_BLOCKS = {}


def blocks_of(name):
    """The host build's blocks of case `name`; deflated once."""
    if name not in _BLOCKS:
        _BLOCKS[name] = bam.bgzf_deflate(dc.parts()[name])
    return _BLOCKS[name]


@pytest.mark.parametrize('name', sorted(dc.parts()))
def test_blocks_give_their_parts_back(name, tmp_path):
    parts, blocks = dc.parts()[name], blocks_of(name)
    assert len(blocks) == len(parts)
    for part, blk in zip(parts, blocks):
        dc.judge(part, blk)
    assert bam.inflate_blocks(blocks, verify=True) == parts
    path = str(tmp_path / 'blocks.gz')
    with open(path, 'wb') as f:
        f.write(b''.join(blocks) + bam.BGZF_EOF)
    assert bam.verify_bgzf(path)['inflated_bytes'] == sum(len(p) for p in parts)
    assert bam.bgzf_deflate(parts) == blocks                   # the same bytes again


def test_size_conditions():
    sizes = {name: (sum(len(p) for p in dc.parts()[name]), sum(len(b) for b in blocks_of(name))) for name in dc.parts()}
    print(sizes)
    for name in ('one_byte', 'chunk'):
        assert 8 * sizes[name][1] < sizes[name][0], name
    for k in range(3):
        n_in, n_out = sizes['pipeline{0}'.format(k)]
        assert 2 * n_out < n_in
    # random bytes come out stored: the block is its input, the BGZF frame and at most 6 bytes for each DEFLATE block
    (part,), (blk,) = dc.parts()['random'], blocks_of('random')
    assert len(part) + 26 < len(blk) <= dc.stored_bound(len(part)) <= 65536
    # the largest allowed distance is used -- random bytes repeat nowhere else, and a table of one position per hash still
    # finds some of the repeats -- and the next larger one is not (zlib would refuse it: the round trip above)
    near, far = blocks_of('distance')
    assert len(near) < len(dc.parts()['distance'][0]) and len(far) > len(dc.parts()['distance'][1])
    # the last match of the straddling input ends on the block's last byte: 100 matches, a period of literals, three headers
    assert len(blocks_of('straddle')[0]) < 101 + 100 * 6 + 4 * 563 + 26


def test_many_blocks_and_none():
    parts = dc.many_parts()
    blocks = bam.bgzf_deflate(parts)
    assert len(blocks) == 3000
    for part, blk in zip(parts[::97], blocks[::97]):
        dc.judge(part, blk)
    assert bam.inflate_blocks(blocks, verify=True) == parts
    assert bam.bgzf_deflate([]) == []


def test_refused_arguments():
    with pytest.raises(ValueError, match='at most 65280'):
        bam.bgzf_deflate([b'ok', b'\x00' * (dc.BLOCK_DATA + 1)])
    lib = _lib.load()
    i64, i32, u8 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8
    data, out, off = np.zeros(100, np.uint8), np.zeros(4096, np.uint8), np.zeros(2, np.int64)

    def host(beg, n, cap=4096, n_data=100):
        return lib.dn_bgzf_deflate_host(_lib._p(data, u8), n_data, 1, _lib._p(np.array([beg], np.int64), i64), _lib._p(np.array([n], np.int32), i32),
                                        _lib._p(out, u8), cap, _lib._p(off, i64))
    assert host(0, 100) == 0 and off[1] > 0
    assert host(0, -1) == _lib.DN_E_INVALID and host(0, dc.BLOCK_DATA + 1, 1 << 20, 1 << 20) == _lib.DN_E_INVALID
    assert host(1, 100) == _lib.DN_E_INVALID and host(-1, 10) == _lib.DN_E_INVALID
    assert host(0, 100, dc.stored_bound(100) - 1) == _lib.DN_E_INVALID and b'out_cap' in lib.dn_last_error()
    assert host(0, 100, dc.stored_bound(100)) == 0
    assert lib.dn_bgzf_deflate_bound(1, _lib._p(np.array([100], np.int32), i32)) == dc.stored_bound(100)
    assert lib.dn_bgzf_deflate_bound(1, _lib._p(np.array([dc.BLOCK_DATA], np.int32), i32)) == dc.stored_bound(dc.BLOCK_DATA) < 65536


# --- the code-length builder ------------------------------------------------------------------------------------------------

def code_lengths(freq, limit):
    freq = np.ascontiguousarray(freq, np.uint32)
    lens = np.full(len(freq), 99, np.uint8)
    rc = _lib.load().dn_deflate_code_lengths_host(_lib._p(freq, ctypes.c_uint32), len(freq), limit, _lib._p(lens, ctypes.c_uint8))
    assert rc == 0
    return lens.astype(np.int64)


def huffman_depths(freq):
    """Depth of every used symbol in a Huffman tree (heapq), and the tree's cost."""
    heap = [(int(f), k, [k]) for k, f in enumerate(freq) if f]
    depth = dict.fromkeys([k for _, k, _ in heap], 0)
    heapq.heapify(heap)
    tick = len(freq)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for k in a + b:
            depth[k] += 1
        tick += 1
        heapq.heappush(heap, (fa + fb, tick, a + b))
    return depth, sum(int(freq[k]) * d for k, d in depth.items())


def frequency_vectors():
    rng = np.random.default_rng(7)
    out = []
    for n in (2, 3, 19, 30, 100, 286):
        out.append(rng.integers(1, 1000, n))                                     # every symbol used
        sparse = rng.integers(0, 5000, n) * (rng.random(n) < 0.5)
        sparse[:2] = (1, 2)
        out.append(sparse)
        out.append((rng.random(n) ** 8 * 60000).astype(np.int64) + (rng.random(n) < 0.7))   # a few heavy symbols, many light
    out.append(np.array(dc.fibonacci_counts()))
    out.append(np.array(dc.fibonacci_counts(30)))                                # an unlimited depth of 29
    return out


@pytest.mark.parametrize('limit', (15, 7))
def test_code_lengths(limit):
    n_optimal = n_limited = 0
    for freq in frequency_vectors():
        if (1 << limit) < len(freq):
            continue
        if limit == 7:
            freq = freq[:19]
        lens = code_lengths(freq, limit)
        used = np.flatnonzero(freq)
        assert lens.max() <= limit and ((lens == 0) == (np.asarray(freq) == 0)).all()
        if len(used) >= 2:
            assert sum(1 << (limit - int(l)) for l in lens[used]) == 1 << limit          # the Kraft sum is exactly 1
        depth, cost = huffman_depths(freq)
        if max(depth.values()) <= limit:
            assert int((np.asarray(freq, np.int64) * lens).sum()) == cost
            n_optimal += 1
        else:
            assert int((np.asarray(freq, np.int64) * lens).sum()) >= cost
            n_limited += 1
    assert n_optimal > 0 and n_limited > 0


def test_code_lengths_of_one_symbol_and_of_none():
    for n in (1, 2, 19, 286):
        for k in (0, n - 1):
            freq = np.zeros(n, np.int64)
            freq[k] = 5
            lens = code_lengths(freq, 15)
            assert lens[k] == 1 and lens.sum() == 1
        assert code_lengths(np.zeros(n, np.int64), 7 if n <= 128 else 15).sum() == 0
    lib = _lib.load()
    assert lib.dn_deflate_code_lengths_host(_lib._p(np.ones(19, np.uint32), ctypes.c_uint32), 19, 4, _lib._p(np.zeros(19, np.uint8), ctypes.c_uint8)) == _lib.DN_E_INVALID


# --- sort_bam(deflate='native') ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_native_sort(name, tmp_path):
    src = str(tmp_path / 'in.bam')
    case = sc.build_case(name, src)
    stream, ends = sc.spec_sorted(case['stream'])
    expect = case['header_out'] + stream
    ref = str(tmp_path / 'zlib.bam')
    bam.sort_bam(src, ref)
    ref_index = dc.resolved(bam.build_index(ref), ref)
    out, again = str(tmp_path / 'out.bam'), str(tmp_path / 'again.bam')
    first = None
    for window_bytes in sc.WINDOWS:
        stats = {}
        assert bam.sort_bam(src, out, window_bytes=window_bytes, overwrite=True, stats=stats, deflate='native') == out
        assert sc.check_layout(out, case['header_out'], ends) == expect, (name, window_bytes)
        assert not os.path.exists(out + '.tmp')
        assert dc.resolved(bam.build_index(out), out) == ref_index
        raw = open(out, 'rb').read()
        first = raw if first is None else first
        assert raw == first                                     # the window size does not show in the file
        head = sum(len(b) for b in bam.bgzf_deflate([case['header_out'][a:a + dc.BLOCK_DATA] for a in range(0, len(case['header_out']), dc.BLOCK_DATA)]))
        assert stats['out_bytes'] == len(raw) - head - len(bam.BGZF_EOF) and stats['deflate_device_ms'] == 0.0
        assert stats['records'] == len(case['rows']) and stats['bytes'] == len(case['stream'])
    bam.sort_bam(src, again, deflate='native')
    assert open(again, 'rb').read() == first                    # two runs write the same bytes
    assert bam.verify_bgzf(out)['inflated_bytes'] == len(expect) and bam.sort_order(out) == 'coordinate'


def test_the_default_did_not_move(tmp_path):
    src = str(tmp_path / 'in.bam')
    case = sc.build_case('three', src)
    stream, ends = sc.spec_sorted(case['stream'])
    hdr = case['header_out']
    expect = b''.join(bam.bgzf_compress(hdr[a:a + dc.BLOCK_DATA], 1) for a in range(0, len(hdr), dc.BLOCK_DATA))
    body = b''.join(bam.bgzf_compress(stream[a:b], 1) for a, b in bam._block_cuts([ends]))
    stats = {}
    for kw in ({}, {'deflate': 'zlib'}):
        out = bam.sort_bam(src, str(tmp_path / 'out.bam'), overwrite=True, stats=stats, **kw)
        assert open(out, 'rb').read() == expect + body + bam.BGZF_EOF
        assert stats['out_bytes'] == len(body) and stats['deflate_device_ms'] == 0.0
    with pytest.raises(ValueError, match="'zlib' or 'native'"):
        bam.sort_bam(src, str(tmp_path / 'x.bam'), deflate='fast')
    assert not os.path.exists(str(tmp_path / 'x.bam'))


def test_failed_native_call_leaves_nothing_behind(tmp_path):
    files = sc.error_files(tmp_path)
    for name in ('ref_range', 'block_size', 'inflate'):
        path, kw, text = files[name]
        dst = str(tmp_path / (name + '_out.bam'))
        with pytest.raises(ValueError) as e:
            bam.sort_bam(path, dst, deflate='native', **kw)
        assert text in str(e.value) and path in str(e.value)
        assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')


def test_sort_deflate_states():
    lib = _lib.load()
    i64, i32, u8 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8
    h = ctypes.c_void_p()
    assert lib.dn_bam_sort_create(-1, 1, 0, 0, 0, ctypes.byref(h)) == 0
    beg, n, out, off = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(64, np.uint8), np.zeros(2, np.int64)
    args = (1, _lib._p(beg, i64), _lib._p(n, i32), _lib._p(out, u8), 64, _lib._p(off, i64), None)
    try:
        assert lib.dn_bam_sort_deflate(h, *args) == _lib.DN_E_STATE                # not finished
        n_rec, n_bytes = i64(0), i64(0)
        assert lib.dn_bam_sort_finish(h, ctypes.byref(n_rec), ctypes.byref(n_bytes), None, None, None, None) == 0
        assert lib.dn_bam_sort_deflate(h, *args) == 0 and off[1] == 28            # an empty range of an empty stream
        n[0] = 1
        assert lib.dn_bam_sort_deflate(h, *args) == _lib.DN_E_INVALID             # a range outside the stream
    finally:
        lib.dn_bam_sort_destroy(h)


def test_command_arguments(tmp_path, monkeypatch):
    from degnorm_amd import __main__ as cli
    from degnorm_amd import pipeline
    assert cli.argparser().parse_args(['--sort-bam', '--native-deflate', '--bam-dir', 'x']).native_deflate
    assert not cli.argparser().parse_args(['--sort-bam', '--bam-dir', 'x']).native_deflate
    src, src2 = str(tmp_path / 'u.bam'), str(tmp_path / 'v.bam')
    sc.build_case('minus_one', src)
    sc.build_case('empty', src2)
    gtf = str(tmp_path / 'g.gtf')
    open(gtf, 'w').write('')

    def args(**kw):
        base = dict(bam_files=[src, src2], bai_files=None, bam_dir=None, warm_start_dir=None, genome_annotation=gtf, output_dir=None,
                    downsample_rate=1, nmf_iter=100, iter=5, minimax_coverage=0, skip_baseline_selection=False,
                    non_unique_alignments=False, proc_per_node=1, create_bai=False, sort_bam=False, native_deflate=False,
                    device_inflate=False, device_frame=False)
        base.update(kw)
        return argparse.Namespace(**base)

    with pytest.raises(ValueError, match='--native-deflate without --sort-bam'):
        cli.validate_args(args(native_deflate=True, create_bai=True))
    seen = []
    monkeypatch.setattr(bam, 'sort_bam', lambda s, d, **kw: seen.append(kw) or d)
    monkeypatch.setattr(bam, 'create_index', lambda b, i, **kw: i)
    monkeypatch.setattr(pipeline, 'run_pipeline', lambda *a, **kw: None)
    for flag in (True, False):
        ok = cli.validate_args(args(sort_bam=True, native_deflate=flag))
        assert ok.sort_bam_files == [src, src2]
        cli._run(ok, str(tmp_path / 'out'), None, False)
        assert [kw['deflate'] for kw in seen[-2:]] == ['native' if flag else 'zlib'] * 2
