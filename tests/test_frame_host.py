"""
Segmented record framing without a GPU: the host build of csrc/dn_frame.hip (bam.frame_records(..., segment_bytes=S)) against
the serial walk (bam.frame_records(buf, tid, last_pos)) on the cases of tests/_frame_cases.py -- equal offsets, bytes consumed
and last pos, equal error texts, no tolerance -- and the frame option of the reader, the pipeline and the command line.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _frame_cases as fc                                      # noqa: E402
from degnorm_amd import bam                                    # noqa: E402


@pytest.fixture(scope='module')
def valid():
    """(name, buf, tid, last_pos, what the serial walk gives) of every valid case; computed once."""
    return [(name, buf, tid, lp, fc.outcome(bam.frame_records, buf, tid, lp)) for name, buf, tid, lp in fc.valid_cases()]


@pytest.mark.parametrize('segment_bytes', fc.SEGMENTS)
def test_valid_cases_equal_serial_walk(valid, segment_bytes):
    for name, buf, tid, lp, expect in valid:
        assert expect[0] == 'ok', name
        stats = {}
        got = fc.outcome(bam.frame_records, buf, tid, lp, segment_bytes=segment_bytes, stats=stats)
        assert got == expect, (name, segment_bytes)
        size = segment_bytes or 16384
        assert stats['segments'] == (len(buf) + size - 1) // size and stats['fixups'] >= 0 and stats['device_ms'] == 0.0
    whole = next(v for v in valid if v[0] == 'whole')
    assert len(whole[4][1]) == 3000 and whole[4][2] == len(whole[1])
    cut = [v for v in valid if v[0].startswith('cut')]
    assert len(cut) == 40 and all(v[4][2] < len(v[1]) for v in cut)            # every cut leaves a carried tail


def test_long_record_leaves_segments_without_an_entry(valid):
    name, buf, tid, lp, expect = next(v for v in valid if v[0] == 'long')
    starts = set(o // 4096 for o in expect[1])
    assert len(set(range(len(buf) // 4096)) - starts) >= 3                      # segments no record starts in


def test_decoys_force_fixups(valid):
    """Without the fix-up path the 'last' decoys cannot frame right: most first-plausible guesses at 256 bytes are decoys."""
    name, buf, tid, lp, expect = next(v for v in valid if v[0] == 'decoy_last')
    stats = {}
    got = fc.outcome(bam.frame_records, buf, tid, lp, segment_bytes=256, stats=stats)
    assert got == expect and len(expect[1]) == 400
    print('decoy_last at 256 bytes: {0} fix-ups in {1} segments'.format(stats['fixups'], stats['segments']))
    assert stats['fixups'] >= 10


@pytest.mark.parametrize('segment_bytes', fc.SEGMENTS)
def test_error_cases_equal_serial_walk(segment_bytes):
    kinds = set()
    for name, buf, tid, lp in fc.error_cases(segment_bytes):
        expect = fc.outcome(bam.frame_records, buf, tid, lp)
        got = fc.outcome(bam.frame_records, buf, tid, lp, segment_bytes=segment_bytes)
        assert got == expect, (name, segment_bytes)
        assert expect[0] == ('ok' if name.endswith('_any_ref') and 'malformed' not in name else 'error'), name
        if expect[0] == 'error':
            kinds.add('malformed' if 'malformed BAM record' in expect[1] else 'sorted' if 'not sorted' in expect[1] else expect[1])
    assert kinds == {'malformed', 'sorted'}
    # the earlier error wins, either way round
    two = {name: fc.outcome(bam.frame_records, buf, tid, lp) for name, buf, tid, lp in fc.error_cases(segment_bytes) if 'then' in name}
    assert 'not sorted' in two['sort_then_malformed'][1] and 'malformed BAM record' in two['malformed_then_sort'][1]


def test_segment_bytes_below_64_is_refused():
    buf = fc.mixed(5, 1)[0]
    with pytest.raises(ValueError, match='segment_bytes'):
        bam.frame_records(buf, 0, fc.INT32_MIN, segment_bytes=63)
    assert fc.outcome(bam.frame_records, buf, 0, fc.INT32_MIN, segment_bytes=64) == fc.outcome(bam.frame_records, buf, 0, fc.INT32_MIN)


def test_frame_option_is_checked(tmp_path):
    with pytest.raises(ValueError, match="frame must be 'host' or 'device', not 'bogus'"):
        bam.NativeBamReadsProcessor('x.bam', 'x.bai', frame='bogus')


def test_device_frame_flag_reaches_run_pipeline(tmp_path, monkeypatch):
    from degnorm_amd import __main__ as cli
    from degnorm_amd import pipeline
    assert cli.argparser().parse_args([]).device_frame is False
    for name in ('a.bam', 'a.bai', 'b.bam', 'b.bai', 'g.gtf'):
        (tmp_path / name).write_bytes(b'')
    seen = []
    monkeypatch.setattr(pipeline, 'run_pipeline', lambda *a, **kw: seen.append(kw))
    base = ['--bam-files', str(tmp_path / 'a.bam'), str(tmp_path / 'b.bam'), '-g', str(tmp_path / 'g.gtf')]
    assert cli.main(base + ['-o', str(tmp_path / 'o1'), '--device-frame']) == 0
    assert cli.main(base + ['-o', str(tmp_path / 'o2'), '--device-frame', '--device-inflate']) == 0
    assert cli.main(base + ['-o', str(tmp_path / 'o3')]) == 0
    assert [(kw['inflate'], kw['frame']) for kw in seen] == [('host', 'device'), ('device', 'device'), ('host', 'host')]
