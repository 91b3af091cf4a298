"""
Host tests of .bai creation (degnorm_amd.bam.build_index with device=None: the host build of csrc/dn_bai.hip; no GPU): the
index against the pure-Python builder of tests/_bai_cases.py byte for byte on every case, block layout, window size and
segment size; its pseudo-bins against the index tests/_bam_fixtures.write_bam computes on its own; region queries against
brute force over the reads and against the specification's reader; parse_bai / tobytes round trips; the errors; create_index,
utils.create_index_file and the command's --create-bai.
"""
import argparse
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bai_cases as bc                                        # noqa: E402
import _bam_fixtures as bf                                     # noqa: E402
from conftest import GOLDEN                                    # noqa: E402
from degnorm_amd import __main__ as cli                        # noqa: E402
from degnorm_amd import bam, utils                             # noqa: E402


@pytest.fixture(scope='module')
def built(tmp_path_factory):
    """{(case, layout): (path, refs, records, blocks, reads, spec bytes)}, each written and specified once."""
    d = tmp_path_factory.mktemp('bai')
    out = {}
    for name in bc.CASES:
        for layout in bc.LAYOUTS:
            p = str(d / '{0}_{1}.bam'.format(name, layout))
            refs, records, blocks, reads = bc.build_case(name, layout, p, level=6 if layout == 'empty' else 1)
            out[name, layout] = (p, refs, records, blocks, reads, bc.spec_index(refs, records, blocks))
    return out


def test_cases_cover_what_they_claim(built):
    p, refs, records, blocks, reads, spec = built['deep', 'aligned']
    levels = set()
    for ref, beg, end, flag, s, e in bc.record_table(records):
        b = bc.reg2bin(beg, end)
        levels.add(sum(b >= first for first in (1, 9, 73, 585, 4681)))
    assert levels == {0, 1, 2, 3, 4, 5}
    assert len(reads) > 2000 and len(blocks) > 20
    # a record that ends exactly at a block's end, an empty block in the file's middle, a header that ends inside a block
    assert any(size == 0 for _, _, size in built['three', 'empty'][3][1:-1])
    ends = set(int(s) for s in records[1][1:])
    assert any(start + size in ends for _, start, size in blocks if size)
    hdr = len(bf.header_bytes(refs))
    assert not any(start == hdr for _, start, _ in built['deep', 'midheader'][3])
    assert not any(start == hdr for _, start, _ in built['deep', 'straddle'][3])


@pytest.mark.parametrize('layout', bc.LAYOUTS)
@pytest.mark.parametrize('name', sorted(bc.CASES))
def test_host_build_equals_specification(built, name, layout):
    p, refs, records, blocks, reads, spec = built[name, layout]
    for window_bytes in bc.WINDOWS:
        for segment_bytes in bc.SEGMENTS:
            stats = {}
            idx = bam.build_index(p, window_bytes=window_bytes, segment_bytes=segment_bytes, n_jobs=2 if window_bytes else 1, stats=stats)
            assert idx.tobytes() == spec, (name, layout, window_bytes, segment_bytes)
            assert stats['records'] == len(reads) and stats['index_device_ms'] == 0.0
            assert stats['chunks'] > 0 and (stats['windows'] == 1 if window_bytes is None else stats['windows'] > (20 if window_bytes == 1 else 3))
    assert idx.n_no_coor == int((reads.ref < 0).sum())


@pytest.mark.parametrize('straddle', [False, True])
@pytest.mark.parametrize('name', sorted(bc.CASES))
def test_pseudo_bins_equal_the_fixture_writers(name, straddle, tmp_path):
    refs, reads = bc.CASES[name]()
    p = str(tmp_path / 'f.bam')
    bf.write_bam(p, refs, reads, straddle=straddle, block_size=30000)
    idx = bam.build_index(p, window_bytes=100000)
    theirs, n_no_coor = bam.read_bai(p + '.bai')
    assert idx.n_no_coor == n_no_coor
    for tid in range(len(refs)):
        assert idx.pseudo(tid) == theirs[tid]['pseudo'], tid
    assert sum(idx.pseudo(t) is not None for t in range(len(refs))) == 2
    # and the written file reads back as what was built
    out = bam.write_bai(idx, str(tmp_path / 'mine.bai'))
    assert bam.parse_bai(out).tobytes() == idx.tobytes()
    mine, _ = bam.read_bai(out)
    assert [m['pseudo'] for m in mine] == [t['pseudo'] for t in theirs]


@pytest.mark.parametrize('name', sorted(bc.CASES))
def test_region_queries(built, name):
    p, refs, records, blocks, reads, spec = built[name, 'straddle']
    idx = bam.build_index(p)
    table = [(ref, beg, end, bc.voffset(blocks, s)) for ref, beg, end, flag, s, e in bc.record_table(records)]
    n_hits = 0
    for tid, beg, end in bc.regions(refs, reads, 200, seed=11):
        chunks = bam.index_chunks(idx, tid, beg, end)
        assert chunks == bc.spec_query(spec, tid, beg, end), (tid, beg, end)
        assert all(a < b for a, b in chunks) and all(x[1] < y[0] for x, y in zip(chunks[:-1], chunks[1:]))
        for ref, rb, re_, vb in table:
            if ref == tid and rb < end and re_ > beg:
                n_hits += 1
                assert any(a <= vb < b for a, b in chunks), (tid, beg, end, rb, re_)
    assert n_hits > 1000


@pytest.mark.parametrize('golden_name', ['hg_small_1', 'hg_small_2', 'ff_small'])
def test_parse_bai_round_trips_the_goldens(golden_name):
    path = os.path.join(GOLDEN, golden_name + '.bai')
    idx = bam.parse_bai(path)
    with open(path, 'rb') as f:
        assert idx.tobytes() == f.read()
    old, n_no_coor = bam.read_bai(path)
    assert len(idx.refs) == len(old) and idx.n_no_coor == n_no_coor
    assert [idx.pseudo(t) for t in range(len(old))] == [o['pseudo'] for o in old]


def test_parse_bai_round_trips_a_fixture_index(tmp_path):
    refs, reads = bc.CASES['three']()
    p = str(tmp_path / 'f.bam')
    bf.write_bam(p, refs, reads)
    with open(p + '.bai', 'rb') as f:
        assert bam.parse_bai(p + '.bai').tobytes() == f.read()
    with pytest.raises(ValueError, match='not a .bai index'):
        bam.parse_bai(p)


def test_errors(tmp_path):
    for name, (path, text) in bc.error_files(tmp_path).items():
        for kw in bc.ERROR_SIZES:
            with pytest.raises(ValueError) as e:
                bam.build_index(path, **kw)
            assert text in str(e.value) and str(e.value).startswith(path + ': '), (name, str(e.value))
    with pytest.raises(ValueError, match='segment_bytes must be at least 64'):
        bam.build_index(path, segment_bytes=8)
    # a block of more than 64 KiB (no BGZF writer makes one): a record that starts behind byte 65535 of it has no virtual offset
    refs, reads = bc.CASES['three']()
    p = str(tmp_path / 'wide.bam')
    bf.write_bam(p, refs, reads, block_size=70000, level=6, index=False)
    assert int(bam.bgzf_blocks(p)[2].max()) > 70000
    with pytest.raises(ValueError, match='starts beyond byte 65535 of its BGZF block'):
        bam.build_index(p)


def test_create_index(built, tmp_path):
    import shutil
    src, refs, records, blocks, reads, spec = built['three', 'aligned']
    p = str(tmp_path / 's.bam')
    shutil.copy(src, p)
    assert bam.create_index(p) == p + '.bai'
    with open(p + '.bai', 'rb') as f:
        assert f.read() == spec
    with pytest.raises(FileExistsError):
        bam.create_index(p)
    open(p + '.bai', 'wb').close()
    assert bam.create_index(p, overwrite=True, window_bytes=50000) == p + '.bai'
    assert bam.parse_bai(p + '.bai').tobytes() == spec
    other = str(tmp_path / 'elsewhere.idx')
    assert bam.create_index(p, other) == other and open(other, 'rb').read() == spec
    # X.bam -> X.bai, the reference's naming
    assert utils.create_index_file(p) == str(tmp_path / 's.bai')
    assert open(str(tmp_path / 's.bai'), 'rb').read() == spec
    with pytest.raises(ValueError, match='.bam extension'):
        utils.create_index_file(other)
    # an error leaves nothing behind: no index and no temporary file
    bad_dir = tmp_path / 'bad'
    bad_dir.mkdir()
    files = bc.error_files(bad_dir)
    before = sorted(os.listdir(str(bad_dir)))
    with pytest.raises(ValueError, match='not sorted by coordinate'):
        bam.create_index(files['pos_order'][0])
    with pytest.raises(OSError):
        bam.create_index(p, str(bad_dir / 'no_such_dir' / 'x.bai'))
    assert sorted(os.listdir(str(bad_dir))) == before
    # the reader accepts what was created
    proc_refs, n_no_coor = bam.read_bai(p + '.bai')
    assert n_no_coor == 150 and bam.reference_range(proc_refs[1]) is None and bam.reference_range(proc_refs[0]) is not None


def _args(**kw):
    base = dict(bam_files=None, bai_files=None, bam_dir=None, warm_start_dir=None, genome_annotation=None, output_dir=None,
                downsample_rate=1, nmf_iter=100, iter=5, minimax_coverage=0, skip_baseline_selection=False,
                non_unique_alignments=False, proc_per_node=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_command_line_flag(tmp_path):
    d = str(tmp_path)
    gtf = os.path.join(d, 'a.gtf')
    open(gtf, 'w').close()
    bams = [os.path.join(d, 's{0}.bam'.format(k)) for k in (1, 2, 3)]
    for b in bams:
        open(b, 'w').close()
    bais = [b[:-3] + 'bai' for b in bams]
    # without the attribute, and with the flag off, the old error
    for kw in ({}, {'create_bai': False}):
        with pytest.raises(FileNotFoundError, match='No .bai index file .*s1.bai'):
            cli.validate_args(_args(bam_files=bams, genome_annotation=gtf, **kw))
        with pytest.raises(FileNotFoundError, match='No .bai index file .*s1.bai'):
            cli.validate_args(_args(bam_dir=d, genome_annotation=gtf, **kw))
    for src in (dict(bam_files=bams), dict(bam_dir=d)):
        ok = cli.validate_args(_args(genome_annotation=gtf, create_bai=True, **src))
        assert ok.bam_files == bams and ok.bai_files == bais and ok.create_bai_files == bams
    open(bais[1], 'w').close()                                  # one index is there
    for src in (dict(bam_files=bams), dict(bam_dir=d)):
        ok = cli.validate_args(_args(genome_annotation=gtf, create_bai=True, **src))
        assert ok.bai_files == bais and ok.create_bai_files == [bams[0], bams[2]]
    for b in bais:
        open(b, 'w').close()
    ok = cli.validate_args(_args(bam_files=bams, genome_annotation=gtf, create_bai=True))
    assert ok.create_bai_files == [] and ok.bai_files == bais
    ok = cli.validate_args(_args(bam_files=bams, genome_annotation=gtf))
    assert ok.create_bai_files == []
    ns = cli.argparser().parse_args(['--bam-dir', d, '-g', gtf, '--create-bai'])
    assert ns.create_bai is True and cli.argparser().parse_args(['--bam-dir', d, '-g', gtf]).create_bai is False
    text = cli.argparser().format_help()
    assert '--create-bai' in text and '.bai' in text
