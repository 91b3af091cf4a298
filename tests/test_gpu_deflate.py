"""
GPU tests of the library's DEFLATE encoder on the device (csrc/dn_deflate.hip, one BGZF block per wavefront): the blocks of
degnorm_amd.bam.bgzf_deflate(device=0) against the host build's byte for byte on the inputs of tests/_deflate_cases.py (which
tests/test_deflate_host.py holds against zlib), the round trip through the device's decoder, sort_bam(device=0,
deflate='native') against the host build file for file, and the pipeline samples written unsorted.  No input here is meant to
fail.

stats['out_bytes'] is the size of the blocks that hold records: the file without its header blocks and its end-of-file block.
Indexes are compared after their virtual offsets are resolved to offsets in the inflated file (_deflate_cases.resolved), as in
the host tests.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bai_cases as bc                                        # noqa: E402
import _bam_fixtures as bf                                     # noqa: E402
import _deflate_cases as dc                                    # noqa: E402
import _sort_cases as sc                                       # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu


def all_parts():
    return [p for name in sorted(dc.parts()) for p in dc.parts()[name]]


def test_device_blocks_equal_host_blocks():
    parts = all_parts()
    host, dev = bam.bgzf_deflate(parts), bam.bgzf_deflate(parts, device=0)
    assert len(dev) == len(parts)
    for k, (part, a, b) in enumerate(zip(parts, host, dev)):
        assert a == b, 'block {0} of {1} input bytes differs from the host build\'s'.format(k, len(part))
        dc.judge(part, b)


def test_more_blocks_than_one_round_of_the_grid():
    parts = dc.many_parts()
    dev = bam.bgzf_deflate(parts, device=0)
    assert dev == bam.bgzf_deflate(parts)
    for part, blk in zip(parts[::97], dev[::97]):
        dc.judge(part, blk)
    assert bam.bgzf_deflate([], device=0) == []


def test_device_round_trip():
    parts = all_parts()
    assert bam.inflate_blocks(bam.bgzf_deflate(parts, device=0), device=0, verify=True) == parts


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_device_native_sort_equals_host_native_sort(name, tmp_path):
    src = str(tmp_path / 'in.bam')
    case = sc.build_case(name, src)
    host, dev = str(tmp_path / 'host.bam'), str(tmp_path / 'dev.bam')
    bam.sort_bam(src, host, deflate='native')
    expect = open(host, 'rb').read()
    assert sc.inflate_file(host)[0] == case['header_out'] + sc.spec_sorted(case['stream'])[0]
    hdr = case['header_out']
    head = sum(len(b) for b in bam.bgzf_deflate([hdr[a:a + dc.BLOCK_DATA] for a in range(0, len(hdr), dc.BLOCK_DATA)]))
    for window_bytes in sc.WINDOWS:
        stats = {}
        bam.sort_bam(src, dev, device=0, window_bytes=window_bytes, overwrite=True, stats=stats, deflate='native')
        assert open(dev, 'rb').read() == expect, (name, window_bytes)
        assert stats['out_bytes'] == len(expect) - head - len(bam.BGZF_EOF)
        assert stats['records'] == len(case['rows']) and stats['bytes'] == len(case['stream'])
        if len(case['rows']):
            assert stats['deflate_device_ms'] > 0
    if name == 'three':
        # a 'zlib' device sort after a 'native' one still equals the host's
        a, b = str(tmp_path / 'a.bam'), str(tmp_path / 'b.bam')
        assert open(bam.sort_bam(src, a, device=0), 'rb').read() == open(bam.sort_bam(src, b), 'rb').read()


def _unsorted_copy(path, refs, rows, seed, straddle):
    """
    The sorted fixture's records in a seeded order that keeps records of equal (refID, pos) in their relative order, under
    SO:unsorted (the idea of tests/test_gpu_sort.py).  Returns the inflated bytes of the sorted fixture.
    """
    rows = bf.sort_reads(rows)
    data, offs = bf.encode_records(rows)
    ends = np.append(offs[1:], len(data))
    perm = np.random.default_rng(seed).permutation(len(rows))
    group = rows.groupby(['ref', 'pos'], sort=False).ngroup().values
    where = np.argsort(perm, kind='stable')
    for g in np.flatnonzero(np.bincount(group) > 1):
        members = np.flatnonzero(group == g)
        where[members] = np.sort(where[members])
    order = np.argsort(where, kind='stable')
    assert (order != np.arange(len(rows))).any()
    shuffled = b''.join(data[offs[k]:ends[k]] for k in order.tolist())
    new_offs = np.concatenate([[0], np.cumsum((ends - offs)[order])[:-1]])
    hdr = bf.header_bytes(refs, text='@HD\tVN:1.6\tSO:unsorted\n')
    bc.write_layout(path, hdr, shuffled, bc.layout_cuts('straddle' if straddle else 'aligned', len(hdr), new_offs, len(shuffled)), 1)
    return bf.header_bytes(refs) + data


def test_pipeline_samples(tmp_path):
    import _gtf_fixtures as gf
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        src, out, ref = (str(tmp_path / (s + e)) for e in ('.bam', '_native.bam', '_zlib.bam'))
        expect = _unsorted_copy(src, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), 40 + k, straddle=(k == 1))
        bam.sort_bam(src, out, device=0, deflate='native')
        assert sc.inflate_file(out)[0] == expect
        bam.sort_bam(src, ref, device=0)
        made = bam.create_index(out, device=0)
        assert dc.resolved(bam.parse_bai(made), out) == dc.resolved(bam.build_index(ref), ref)
