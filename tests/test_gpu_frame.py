"""
GPU tests of segmented record framing (csrc/dn_frame.hip) and of NativeBamReadsProcessor(frame='device'): the cases of
tests/_frame_cases.py on the device against the serial host walk (equal offsets and equal error texts; the error inputs go to
the device only after the valid ones have passed in this run and the host build has given the expected error), and the
device-framing reader against the host-framing reader, with either inflate, on the goldens, small windows with trimmed index
ranges, the filter cases, a several-window scale case, an unsorted and a malformed file and the BAM + GTF pipeline.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _frame_cases as fc                                      # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_reads import _case                               # noqa: E402
from test_gpu_bam import _files, _layout_case, _run, _same     # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = set()                                          # segment sizes whose valid cases have passed in this run


@pytest.fixture(scope='module')
def valid():
    return [(name, buf, tid, lp, fc.outcome(bam.frame_records, buf, tid, lp)) for name, buf, tid, lp in fc.valid_cases()]


@pytest.mark.parametrize('segment_bytes', fc.SEGMENTS)
def test_valid_cases_equal_serial_walk(valid, segment_bytes):
    for name, buf, tid, lp, expect in valid:
        stats = {}
        got = fc.outcome(bam.frame_records, buf, tid, lp, device=0, segment_bytes=segment_bytes, stats=stats)
        assert expect[0] == 'ok' and got == expect, (name, segment_bytes)
        if name == 'whole':
            assert stats['device_ms'] > 0 and stats['segments'] > 0
        if name == 'decoy_last' and segment_bytes == 256:
            print('decoy_last at 256 bytes: {0} fix-ups in {1} segments'.format(stats['fixups'], stats['segments']))
            assert stats['fixups'] >= 10
    _VALID_PASSED.add(segment_bytes)


@pytest.mark.parametrize('segment_bytes', fc.SEGMENTS)
def test_error_cases_equal_serial_walk(valid, segment_bytes):
    assert segment_bytes in _VALID_PASSED, 'no error input goes to the device before the valid cases of this size have passed in this run'
    for name, buf, tid, lp in fc.error_cases(segment_bytes):
        expect = fc.outcome(bam.frame_records, buf, tid, lp)
        assert fc.outcome(bam.frame_records, buf, tid, lp, segment_bytes=segment_bytes) == expect, name      # the host build first
        assert fc.outcome(bam.frame_records, buf, tid, lp, device=0, segment_bytes=segment_bytes) == expect, (name, segment_bytes)
    # a call after an error works
    name, buf, tid, lp, expect = valid[0]
    assert fc.outcome(bam.frame_records, buf, tid, lp, device=0, segment_bytes=segment_bytes) == expect


def _all_modes(path, chrom, ov, gene_df, exon_df, out, **kw):
    """frame='host' and frame='device' with either inflate: output files and load_chromosome_reads frames must be identical."""
    res = {}
    for inflate in ('host', 'device'):
        for frame in ('host', 'device'):
            proc, files = _run(path, chrom, ov, gene_df, exon_df, os.path.join(str(out), inflate + '_' + frame), inflate=inflate,
                               frame=frame, **kw)
            res[inflate, frame] = (proc, files, proc.load_chromosome_reads(chrom))
        _same(res[inflate, 'host'][1], res[inflate, 'device'][1])
        pd.testing.assert_frame_equal(res[inflate, 'host'][2], res[inflate, 'device'][2])
        t = res[inflate, 'device'][0].timing
        assert t['frame_device_ms'] > 0 and 'frame_s' not in t and t['frame_fixups'] >= 0
        assert 'frame_device_ms' not in res[inflate, 'host'][0].timing
    return res


TIMING_KEYS = {('host', 'host'): {'inflate_s', 'frame_s', 'decode_s'},
               ('device', 'host'): {'inflate_s', 'inflate_device_ms', 'frame_s', 'decode_s'},
               ('host', 'device'): {'inflate_s', 'upload_s', 'frame_device_ms', 'frame_fixups', 'decode_s'},
               ('device', 'device'): {'inflate_s', 'inflate_device_ms', 'frame_device_ms', 'frame_fixups', 'decode_s'}}


def test_one_ingest_loop_serves_the_four_combinations(tmp_path):
    """Windows of 64 KiB over a single-end file: every combination carries cut records, gives host / host's outputs and keeps its timing keys."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(21, 4000, False)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values})
    p = str(tmp_path / 'se.bam')
    bf.write_bam(p, [(chrom, chrom_len)], df, straddle=True)
    kw = {'window_bytes': 1 << 16}
    res = {}
    for inflate in ('host', 'device'):
        for frame in ('host', 'device'):
            proc, files = _run(p, chrom, ov, gene_df, exon_df, tmp_path / (inflate + '_' + frame), inflate=inflate, frame=frame, **kw)
            assert not proc.paired
            res[inflate, frame] = files
            _same(res['host', 'host'], files)
            assert set(proc.timing) == TIMING_KEYS[inflate, frame] | {'coverage_s', 'coverage_device_ms'}, (inflate, frame)
    assert int(res['host', 'host'][2].iloc[:, 1].sum()) > 1000
    assert len(list(proc._batches(chrom))) > 3
    carry, last, cut = b'', -2 ** 31, 0                          # the host walk over the same windows: records are cut by window ends
    for win in proc.windows(chrom):
        off, used, last = bam.frame_records(carry + win, 0, last)
        cut += used < len(carry + win)
        carry = (carry + win)[used:]
    assert cut > 0 and not carry


@pytest.mark.parametrize('straddle', [False, True])
@pytest.mark.parametrize('key', ['se', 'pe'])
def test_reader_equals_host_framing_on_goldens(key, straddle, tmp_path):
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
    bf.write_bam(p, [('c', chrom_len)], df, straddle=straddle)
    res = _all_modes(p, 'c', ov, gene_df, exon_df, tmp_path)
    assert res['device', 'device'][0].paired == paired and len(res['device', 'device'][2]) > 100


@pytest.mark.parametrize('window_bytes', [1, 70000, None])
def test_windows_carry_and_trims(window_bytes, tmp_path):
    """The three-reference file of test_gpu_inflate: the carried record stays on the device, head and tail are trimmed."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(21, 4000, True)
    df = pd.DataFrame({'ref': 1, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values, 'next_ref': 1})
    before = df.sample(700, random_state=1).assign(ref=0)
    after = df.sample(600, random_state=2).assign(ref=2, qname=lambda d: 'z' + d.qname)
    p = str(tmp_path / 'three.bam')
    bf.write_bam(p, [('chrA', chrom_len), (chrom, chrom_len), ('chrZ', chrom_len)], pd.concat([df, before, after]), straddle=True, level=6)
    vbeg, vend = bam.reference_range(bam.read_bai(p + '.bai')[0][1])
    assert vbeg & 0xffff and vend & 0xffff and (vend >> 16) > (vbeg >> 16)
    kw = {} if window_bytes is None else {'window_bytes': window_bytes}
    res = _all_modes(p, chrom, ov, gene_df, exon_df, tmp_path, chroms=[chrom], **kw)
    assert len(res['device', 'device'][2]) > 1000


@pytest.mark.parametrize('paired,unique', [(False, True), (True, False)])
def test_filter_cases(paired, unique, tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(7, 1500, paired)
    rng = np.random.default_rng(3)
    n = len(src)
    df = pd.DataFrame({'ref': 1, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values,
                       'nh': rng.choice([1, 2, 3, 1, None], n).tolist(), 'nh_type': rng.choice(['C', 'S', 'i', 'c', 's', 'I'], n).tolist(),
                       'next_ref': np.where(rng.random(n) < 0.1, -1, 1)})
    other = df.sample(400, random_state=1).assign(ref=0)
    other2 = df.sample(300, random_state=2).assign(ref=2, qname=lambda d: 'z' + d.qname)
    p = str(tmp_path / 'f.bam')
    bf.write_bam(p, [('chrA', chrom_len), (chrom, chrom_len), ('chrZ', chrom_len)], pd.concat([df, other, other2]), straddle=True)
    got = {}
    for inflate in ('host', 'device'):
        for frame in ('host', 'device'):
            proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / (inflate + frame)), unique_alignment=unique,
                                               chroms=[chrom], verbose=False, inflate=inflate, frame=frame)
            proc.paired = paired
            frame_df = proc.load_chromosome_reads(chrom)
            os.makedirs(proc.save_dir)
            proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
            got[inflate, frame] = (frame_df, _files(proc, chrom))
        pd.testing.assert_frame_equal(got[inflate, 'host'][0], got[inflate, 'device'][0])
        _same(got[inflate, 'host'][1], got[inflate, 'device'][1])
    assert 0 < len(got['device', 'device'][0]) <= n


def test_several_windows_of_many_segments_repeat(tmp_path):
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case(n_reads=100_000)
    df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
    p = str(tmp_path / 'big.bam')
    bf.write_bam(p, [('chrS', chrom_len)], df)
    kw = {'window_bytes': 8 << 20}
    _, host = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / 'host', **kw)
    assert int(host[2].iloc[:, 1].sum()) > 50000
    for inflate in ('host', 'device'):
        proc, dev1 = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / (inflate + '1'), inflate=inflate, frame='device', **kw)
        _, dev2 = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / (inflate + '2'), inflate=inflate, frame='device', **kw)
        _same(host, dev1)
        _same(dev1, dev2)
        assert len(list(proc._batches('chrS'))) > 1


def _host_error(path, chrom, tmp_path):
    with pytest.raises(ValueError) as e:
        bam.NativeBamReadsProcessor(path, path + '.bai', output_dir=str(tmp_path / 'h'), verbose=False).load_chromosome_reads(chrom)
    return str(e.value)


def _two_chromosomes(tmp_path, name, seed):
    """chrG (clean, first: the constructor's look at the first reads stays clean) and a second chromosome, small blocks."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(seed, 3000, False)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values})
    good = df.assign(qname=lambda d: 'g' + d.qname)
    p = str(tmp_path / name)
    bf.write_bam(p, [('chrG', chrom_len), (chrom, chrom_len)], pd.concat([df.assign(ref=1), good]), block_size=20000, level=6)
    return p, chrom, len(good)


def _rewrite_block(p, change):
    """Inflate the middle block of the second chromosome's index range, apply change(bytearray), deflate it to the same place."""
    offs, sizes, _ = bam.bgzf_blocks(p)
    vbeg, vend = bam.reference_range(bam.read_bai(p + '.bai')[0][1])
    inside = [k for k in range(len(offs)) if (vbeg >> 16) < offs[k] < (vend >> 16)]
    k = inside[len(inside) // 2]
    raw = open(p, 'rb').read()
    data = bytearray(bam.inflate_block(raw[offs[k]:offs[k] + sizes[k]]))
    change(data)
    new = bf._bgzf_block(bytes(data), 6)
    with open(p, 'wb') as f:
        f.write(raw[:offs[k]] + new + raw[offs[k] + sizes[k]:])
    # the blocks behind it move by the change in size, and with them the virtual offset the index range ends at
    moved = ((vend >> 16) + len(new) - int(sizes[k])) << 16 | (vend & 0xffff)
    bai = open(p + '.bai', 'rb').read().replace(vend.to_bytes(8, 'little'), moved.to_bytes(8, 'little'))
    with open(p + '.bai', 'wb') as f:
        f.write(bai)
    assert bam.reference_range(bam.read_bai(p + '.bai')[0][1]) == (vbeg, moved)


@pytest.mark.parametrize('kind', ['unsorted', 'malformed'])
def test_bad_file_raises_the_host_text(kind, tmp_path):
    p, chrom, n_good = _two_chromosomes(tmp_path, kind + '.bam', 31)

    def change(data):
        off = bam.frame_records(bytes(data))[0]                         # without straddle a block starts at a record
        at = int(off[len(off) // 2])
        if kind == 'unsorted':
            data[at + 8:at + 12] = (0).to_bytes(4, 'little')            # pos 0 after larger ones, under a valid index
        else:
            data[at:at + 4] = (7).to_bytes(4, 'little')

    _rewrite_block(p, change)
    expect = _host_error(p, chrom, tmp_path)
    assert ('not sorted by coordinate' if kind == 'unsorted' else 'malformed BAM record') in expect
    for inflate in ('host', 'device'):
        proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / inflate), verbose=False, inflate=inflate, frame='device')
        with pytest.raises(ValueError) as e:
            proc.load_chromosome_reads(chrom)
        assert str(e.value) == expect
        assert len(proc.load_chromosome_reads('chrG')) == n_good        # the other chromosome still reads


def test_pipeline_with_device_inflate_and_frame_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, assert_same_table, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.nmf import GeneNMFOA
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
        inflate='device', frame='device')
    assert sample_ids == samples
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_cov(cov, cov_e)
    ref = GeneNMFOA(degnorm_iter=ITER, nmf_iter=NMF_ITER)
    est_e = ref.run(cov_e, reads_dat=counts_e[samples].values.astype(np.float64))
    np.testing.assert_array_equal(model.rho, ref.rho)
    np.testing.assert_array_equal(model.x_adj, ref.x_adj)
    for a, b in zip(estimates, est_e):
        np.testing.assert_array_equal(a, b)
    assert all(os.path.isfile(os.path.join(out, name)) for name in RESULT_FILES)
