"""
Host tests (no GPU) of the coordinate sort of BAM files, degnorm_amd.bam.sort_bam(device=None): the host build of
csrc/dn_sort.hip behind zlib, against the definition of include/degnorm_amd.h stated in plain Python (tests/_sort_cases.py),
byte for byte on the inflated output; the rules of the written blocks; the index of the output; the header rewrite; the
refused files; and the command's --sort-bam arguments.
"""
import argparse
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _sort_cases as sc                                       # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

_BUILT = {}


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    """name -> (path, the case, the expected inflated output, the ends of its records); built once, read only."""
    def get(name):
        if name not in _BUILT:
            p = str(tmp_path_factory.mktemp('sort_' + name) / 'in.bam')
            case = sc.build_case(name, p)
            stream, ends = sc.spec_sorted(case['stream'])
            _BUILT[name] = (p, case, case['header_out'] + stream, ends)
        return _BUILT[name]
    return get


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_sorted_stream_equals_the_definition(name, cases, tmp_path):
    src, case, expect, ends = cases(name)
    rows = case['rows']
    out = str(tmp_path / 'out.bam')
    for window_bytes in sc.WINDOWS:
        for segment_bytes in sc.SEGMENTS:
            stats = {}
            assert bam.sort_bam(src, out, window_bytes=window_bytes, segment_bytes=segment_bytes, overwrite=True, stats=stats) == out
            got = sc.check_layout(out, case['header_out'], ends)
            assert got == expect, (name, window_bytes, segment_bytes)
            assert stats['records'] == len(rows) and stats['bytes'] == len(case['stream']) and stats['windows'] >= 1
            assert not os.path.exists(out + '.tmp')
    assert bam.sort_order(src) != 'coordinate' and bam.sort_order(out) == 'coordinate'
    assert bam.verify_bgzf(out)['inflated_bytes'] == len(expect)
    # the index of the output counts what the rows hold
    idx = bam.build_index(out)
    ref, flag = rows['ref'].values.astype(np.int64), rows['flag'].values.astype(np.int64)
    assert idx.n_no_coor == int((ref < 0).sum())
    for tid in range(len(case['refs'])):
        n_unmapped = int(((ref == tid) & ((flag & 4) != 0)).sum())
        n_mapped = int((ref == tid).sum()) - n_unmapped
        assert (idx.pseudo(tid) or (0, 0, 0, 0))[2:] == (n_mapped, n_unmapped)
    # sorting the output again changes nothing
    again = str(tmp_path / 'again.bam')
    bam.sort_bam(out, again, window_bytes=4096)
    assert sc.inflate_file(again)[0] == expect


def test_output_does_not_depend_on_threads_and_level_is_used(cases, tmp_path):
    src, case, expect, ends = cases('three')
    a, b, c = (str(tmp_path / n) for n in ('a.bam', 'b.bam', 'c.bam'))
    bam.sort_bam(src, a, n_jobs=1)
    bam.sort_bam(src, b, n_jobs=3, window_bytes=70000)
    bam.sort_bam(src, c, level=6)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert os.path.getsize(c) < os.path.getsize(a) and sc.inflate_file(c)[0] == expect


@pytest.mark.parametrize('form', sorted(sc.HEADERS))
def test_header_rewrite(form):
    hdr_in, hdr_out = sc.header_pair(sc.REFS, form, '@PG\tID:aligner\tPN:aligner\n@CO\tSO:unsorted in a comment stays\n')
    assert bam.coordinate_header(hdr_in) == hdr_out
    assert bam.coordinate_header(hdr_out) == hdr_out
    l_text = struct.unpack_from('<i', hdr_out, 4)[0]
    assert bam.parse_header(hdr_out) == (len(hdr_out), sc.REFS) and hdr_out[8 + l_text:] == hdr_in[8 + struct.unpack_from('<i', hdr_in, 4)[0]:]


def test_header_rewrite_without_so_field_and_without_text():
    refs = [('c', 10)]
    with_hd = bf.header_bytes(refs, text='@HD\tVN:1.4\n')
    assert bam.coordinate_header(with_hd) == bf.header_bytes(refs, text='@HD\tVN:1.4\tSO:coordinate\n')
    empty = b'BAM\x01' + struct.pack('<i', 0) + with_hd[8 + struct.unpack_from('<i', with_hd, 4)[0]:]
    got = bam.coordinate_header(empty)
    assert got[8:8 + struct.unpack_from('<i', got, 4)[0]] == sc.HD_OUT.encode() and bam.parse_header(got)[1] == refs


def test_refused_files_leave_nothing_behind(tmp_path):
    for name, (path, kw, text) in sc.error_files(tmp_path).items():
        for sizes in ({}, {'window_bytes': 1, 'segment_bytes': 256}):
            dst = str(tmp_path / (name + '_out.bam'))
            with pytest.raises(ValueError) as e:
                bam.sort_bam(path, dst, **dict(kw, **sizes))
            assert text in str(e.value) and path in str(e.value), (name, str(e.value))
            assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')
    # the flipped bit passes unnoticed without verify: the file is sorted as it is
    path, kw, _ = sc.error_files(tmp_path)['crc']
    assert bam.sort_bam(path, str(tmp_path / 'unchecked.bam')) and bam.sort_order(str(tmp_path / 'unchecked.bam')) == 'coordinate'


def test_existing_destination(cases, tmp_path):
    src = cases('empty')[0]
    dst = str(tmp_path / 'there.bam')
    open(dst, 'wb').write(b'kept')
    with pytest.raises(FileExistsError, match='overwrite=True'):
        bam.sort_bam(src, dst)
    assert open(dst, 'rb').read() == b'kept' and not os.path.exists(dst + '.tmp')
    assert bam.sort_bam(src, dst, overwrite=True) == dst and bam.sort_order(dst) == 'coordinate'
    with pytest.raises(ValueError, match='segment_bytes'):
        bam.sort_bam(src, str(tmp_path / 'x.bam'), segment_bytes=10)


def test_sort_bam_file_names_the_output(cases, tmp_path):
    from degnorm_amd.utils import sort_bam_file
    src = str(tmp_path / 'S1.bam')
    open(src, 'wb').write(open(cases('minus_one')[0], 'rb').read())
    assert sort_bam_file(src) == str(tmp_path / 'S1_sorted.bam') and bam.sort_order(str(tmp_path / 'S1_sorted.bam')) == 'coordinate'
    (tmp_path / 'o').mkdir()
    assert sort_bam_file(src, out_dir=str(tmp_path / 'o'), level=6) == str(tmp_path / 'o' / 'S1_sorted.bam')
    with pytest.raises(ValueError, match='.bam extension'):
        sort_bam_file(str(tmp_path / 'S1.sam'))


def test_command_arguments(cases, tmp_path):
    from degnorm_amd import __main__ as cli
    gtf = str(tmp_path / 'g.gtf')
    open(gtf, 'w').write('')
    unsorted = str(tmp_path / 'u.bam')
    open(unsorted, 'wb').write(open(cases('minus_one')[0], 'rb').read())
    done = str(tmp_path / 'd.bam')
    bam.sort_bam(unsorted, done)

    def args(**kw):
        base = dict(bam_files=None, bai_files=None, bam_dir=None, warm_start_dir=None, genome_annotation=gtf, output_dir=None,
                    downsample_rate=1, nmf_iter=100, iter=5, minimax_coverage=0, skip_baseline_selection=False,
                    non_unique_alignments=False, proc_per_node=1, create_bai=False, sort_bam=False)
        base.update(kw)
        return argparse.Namespace(**base)

    assert cli.argparser().parse_args(['--sort-bam', '--bam-dir', 'x']).sort_bam
    with pytest.raises(ValueError, match='--sort-bam and --bai-files'):
        cli.validate_args(args(bam_files=[unsorted, done], bai_files=['a.bai', 'b.bai'], sort_bam=True))
    # the sorted file is used as it is and needs its index; the unsorted one gets its index later
    with pytest.raises(FileNotFoundError, match='No .bai index file'):
        cli.validate_args(args(bam_files=[unsorted, done], sort_bam=True))
    ok = cli.validate_args(args(bam_files=[unsorted, done], sort_bam=True, create_bai=True))
    assert ok.sort_bam_files == [unsorted] and ok.create_bai_files == [done] and ok.bai_files == [None, done[:-3] + 'bai']
    bam.create_index(done, done[:-3] + 'bai')
    ok = cli.validate_args(args(bam_dir=str(tmp_path), sort_bam=True))
    assert ok.bam_files == [done, unsorted] and ok.sort_bam_files == [unsorted] and ok.create_bai_files == []
    # without the flag nothing is sorted: the unsorted file only lacks its index
    with pytest.raises(FileNotFoundError, match='No .bai index file'):
        cli.validate_args(args(bam_files=[unsorted, done]))
    assert cli.validate_args(args(bam_files=[unsorted, done], create_bai=True)).sort_bam_files == []
