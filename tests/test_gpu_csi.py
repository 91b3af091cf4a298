"""
GPU tests of the .csi index on the device (csrc/dn_bai.hip, degnorm_amd.bam.build_index(device=0, fmt='csi')): the cases,
layouts and window sizes of tests/test_csi_host.py against the host build byte for byte (which that file holds against the
pure-Python specification), streams of 1, 255, 256 and 257 records, the range errors (sent to the device only after the
valid cases have passed in this run); the reader on a created .csi against the reader on the fixture writer's .bai; a
reference beyond 2^29 bases from SAM text to the reads the reader loads; and `python -m degnorm_amd --create-bai
--index-format csi` on the pipeline samples against tests/golden/pipeline.npz.
"""
import os
import pickle
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bai_cases as bc                                        # noqa: E402
import _bam_fixtures as bf                                     # noqa: E402
import _csi_cases as cc                                        # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
import _reads_oracle as ro                                     # noqa: E402
import _sam_cases as sc                                        # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_reads import _case                               # noqa: E402
from test_gpu_bam import _files, _same, expected_frame         # noqa: E402
from degnorm_amd import bam                                    # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure   # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = cc.SHARED + [(name, cc.CASES[name][0], cc.CASES[name][1]) for name in sorted(cc.CASES)]
_VALID_PASSED = set()                                          # (case, min_shift, depth, layout) whose device index equalled the host's


@pytest.mark.parametrize('layout', bc.LAYOUTS)
@pytest.mark.parametrize('name,min_shift,depth', PARAMS)
def test_device_build_equals_host_build(name, min_shift, depth, layout, tmp_path):
    p = str(tmp_path / 'c.bam')
    refs, records, blocks, reads = cc.build_case(name, layout, p, level=6 if layout == 'empty' else 1)
    kw = dict(fmt='csi', min_shift=min_shift, depth=depth)
    expect = bam.build_index(p, **kw).tobytes()
    assert len(expect) > 1000 and expect[:4] == b'CSI\x01'
    for window_bytes in bc.WINDOWS:
        stats = {}
        got = bam.build_index(p, device=0, window_bytes=window_bytes, stats=stats, **kw)
        assert got.tobytes() == expect, (name, layout, window_bytes)
        assert stats['index_device_ms'] > 0 and stats['records'] == len(reads) and stats['chunks'] > 0
        assert stats['windows'] == 1 if window_bytes is None else stats['windows'] > (20 if window_bytes == 1 else 3)
    _VALID_PASSED.add((name, min_shift, depth, layout))


@pytest.mark.parametrize('n', cc.COUNTS)
def test_streams_around_one_workgroup(n, tmp_path):
    p = str(tmp_path / 'n.bam')
    refs, records, blocks, reads = cc.build_case(('count', n), 'aligned', p)
    assert len(reads) == n
    for kw in (dict(depth=None), dict(min_shift=6, depth=8), dict(min_shift=30, depth=1)):
        expect = bam.build_index(p, fmt='csi', **kw)
        assert expect.tobytes() == cc.spec_index(refs, records, blocks, kw.get('min_shift', 14), expect.depth)
        assert bam.build_index(p, device=0, fmt='csi', **kw).tobytes() == expect.tobytes(), (n, kw)


def test_errors_equal_the_host_texts(tmp_path):
    assert len(_VALID_PASSED) == len(PARAMS) * len(bc.LAYOUTS), 'no error input goes to the device before the valid cases have passed in this run'
    for min_shift, depth in cc.RANGE_PARAMS:
        kw = dict(fmt='csi', min_shift=min_shift, depth=depth)
        p = str(tmp_path / 'at_{0}_{1}.bam'.format(min_shift, depth))
        cc.range_file(p, min_shift, depth, 0)
        assert bam.build_index(p, device=0, **kw).tobytes() == bam.build_index(p, **kw).tobytes()       # an end at the cap is held
        p = str(tmp_path / 'past_{0}_{1}.bam'.format(min_shift, depth))
        pos, text = cc.range_file(p, min_shift, depth, 1)
        for sizes in bc.ERROR_SIZES:
            with pytest.raises(ValueError) as host:
                bam.build_index(p, **kw, **sizes)
            assert str(host.value) == text                            # the host build first
            with pytest.raises(ValueError) as dev:
                bam.build_index(p, device=0, **kw, **sizes)
            assert str(dev.value) == text, (min_shift, depth, sizes)
    # the other faults have the texts of the .bai builder, whose own have not moved
    for name, (path, text) in bc.error_files(tmp_path).items():
        with pytest.raises(ValueError) as dev:
            bam.build_index(path, device=0, fmt='bai')
        assert text in str(dev.value), name
        if name != 'beyond':
            with pytest.raises(ValueError) as host:
                bam.build_index(path, fmt='csi')
            with pytest.raises(ValueError) as dev:
                bam.build_index(path, device=0, fmt='csi')
            assert text in str(host.value) and str(dev.value) == str(host.value), name
    with pytest.raises(ValueError, match='min_shift must be 1 .. 30'):
        bam.build_index(path, device=0, fmt='csi', min_shift=0)
    # a valid call after an error works
    p = str(tmp_path / 'ok.bam')
    cc.build_case('levels', 'straddle', p)
    assert bam.build_index(p, device=0, fmt='csi', min_shift=4, depth=3).tobytes() == bam.build_index(p, fmt='csi', min_shift=4, depth=3).tobytes()


def _run(path, index, chrom, ov, gene_df, exon_df, out, **kw):
    proc = bam.NativeBamReadsProcessor(path, index, output_dir=str(out), verbose=False, **kw)
    os.makedirs(proc.save_dir, exist_ok=True)
    proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
    return proc, _files(proc, chrom)


@pytest.mark.parametrize('key', ['se', 'pe'])
def test_reader_on_created_csi_equals_reader_on_fixture_index(key, tmp_path):
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
    (tmp_path / 'theirs').mkdir()
    (tmp_path / 'ours').mkdir()
    theirs, ours = str(tmp_path / 'theirs' / (key + '.bam')), str(tmp_path / 'ours' / (key + '.bam'))
    bf.write_bam(theirs, [('c', chrom_len)], df, straddle=True)
    bf.write_bam(ours, [('c', chrom_len)], df, straddle=True, index=False)
    assert bam.create_index(ours, device=0, fmt='csi') == ours + '.csi' and not os.path.exists(ours + '.bai')
    assert bam.parse_csi(ours + '.csi').pseudo(0) == bam.read_bai(theirs + '.bai')[0][0]['pseudo']
    assert bam.read_index(ours + '.csi')[0][0]['pseudo'] == bam.read_bai(theirs + '.bai')[0][0]['pseudo']
    for inflate, frame in (('host', 'host'), ('device', 'device')):
        _, a = _run(theirs, theirs + '.bai', 'c', ov, gene_df, exon_df, tmp_path / 'theirs' / inflate, inflate=inflate, frame=frame)
        proc, b = _run(ours, ours + '.csi', 'c', ov, gene_df, exon_df, tmp_path / 'ours' / inflate, inflate=inflate, frame=frame)
        _same(a, b)
        assert proc.paired == paired and int(b[2].iloc[:, 1].sum()) > 100


def test_beyond_2_29_from_sam_text_to_loaded_reads(tmp_path):
    """
    Case `beyond` as unsorted SAM text: converted, sorted and indexed (.csi) on the device, the reader loads every read of the
    long reference with its position; a .bai of the same sorted file is still refused.  Then the coverage of one gene of
    three exons across 2^29 against the restatement of tests/_reads_oracle.py, on the case's mapped reads (the restatement
    reads no record without a CIGAR).  Measured once on an MI355X: 0.24 s for the coverage step (7.8 ms on the device),
    1.8 s for the restatement, which holds whole-chromosome vectors of 2^29 + 2^16 entries.
    """
    refs, rows = cc.CASES['beyond'][2]()
    rows = rows.assign(nh=1, nh_type='C')
    lines = sc.sam_text(rows, refs).split(b'\n')[:-1]
    header = '@HD\tVN:1.6\tSO:unsorted\n' + ''.join('@SQ\tSN:{0}\tLN:{1}\n'.format(nm, ln) for nm, ln in refs)
    src = sc.write_sam(str(tmp_path / 'b.sam'), b''.join(lines[k] + b'\n' for k in sc.shuffled_order(rows, 7)), header)
    conv = bam.sam_to_bam(src, str(tmp_path / 'b.bam'), device=0)
    srt = bam.sort_bam(conv, str(tmp_path / 'b_sorted.bam'), device=0)
    assert bam.sort_order(conv) == 'unsorted' and bam.sort_order(srt) == 'coordinate'
    with pytest.raises(ValueError, match='reaches beyond position 2\\^29: a .bai index cannot hold it'):
        bam.create_index(srt, device=0, fmt='bai')
    assert not os.path.exists(srt + '.bai')
    assert bam.create_index(srt, device=0, fmt='csi') == srt + '.csi'
    idx = bam.parse_csi(srt + '.csi')
    assert idx.depth == 6 and idx.tobytes() == bam.build_index(srt, fmt='csi').tobytes()
    proc = bam.NativeBamReadsProcessor(srt, srt + '.csi', verbose=False)
    for tid, chrom in enumerate(('chrH', 'chrS')):
        got, want = proc.load_chromosome_reads(chrom), expected_frame(rows, tid, True, False)
        pd.testing.assert_frame_equal(got, want)
    got = proc.load_chromosome_reads('chrH')
    assert len(got) == int((rows.ref == 0).sum()) > 2000 and int(got.pos.max()) == refs[0][1] - 1 
    # the case puts 20 flag-4 reads, four named ones and what its random draws give at or beyond 2^29
    assert int((got.pos >= 1 << 29).sum()) == int(((rows.ref == 0) & (rows.pos >= 1 << 29)).sum()) >= 24
    # region queries on the written index find the reads beyond 2^29
    chunks = bam.index_chunks(idx, 0, 1 << 29, refs[0][1])
    assert chunks and chunks[0][0] > idx.pseudo(0)[0] and chunks[-1][1] <= idx.pseudo(0)[1]


    # one gene of three exons across 2^29
    mapped = rows[rows.flag == 0].reset_index(drop=True)
    H = 1 << 29
    gene_df, exon_df = rf.tables('chrH', [('G', [(H - 30000, H - 15000), (H - 500, H + 500), (H + 15000, H + 30000)])])
    ov = get_gene_overlap_structure(gene_df)
    p = str(tmp_path / 'm.bam')
    bf.write_bam(p, refs, mapped, index=False)
    bam.create_index(p, device=0, fmt='csi')
    proc = bam.NativeBamReadsProcessor(p, p + '.csi', output_dir=str(tmp_path / 'cov'), verbose=False)
    os.makedirs(proc.save_dir, exist_ok=True)
    proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, 'chrH')
    csr, ol, cnt = _files(proc, 'chrH')
    want = ro.restate(expected_frame(mapped, 0, True, False), refs[0][1], ov, gene_df, exon_df, False)
    ro.assert_same((csr, ol or {}, dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int)))), want, 'beyond')
    assert want[2]['G'] > 20 and csr.indices.min() < H <= csr.indices.max()


def test_command_creates_csi_indexes_and_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.nmf import GeneNMFOA
    paths = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.bam'))
        bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1), index=False)
        paths.append(p)
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    all_cov, _, all_counts, _ = golden_inputs(z, [])
    out = str(tmp_path / 'out')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--create-bai', '--index-format', 'csi', '--device-inflate', '--device-frame', '--bam-files'] + \
        paths + ['-g', GTF, '-o', out, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    for p in paths:
        idx = bam.parse_csi(p[:-3] + 'csi')
        assert idx.tobytes() == bam.build_index(p, fmt='csi').tobytes() and len(idx.refs) == len(gf.PIPELINE_REFS)
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(('.bai', '.csi'))) == sorted(s + '.csi' for s in gf.PIPELINE_SAMPLES)
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'gene_exon_metadata.csv')), golden_frame(z, 'exon', RUN_COLS).reset_index(drop=True))
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'read_counts.csv')), all_counts)
    for c in z['chroms'].tolist():
        with open(os.path.join(out, c, 'coverage_matrices_{0}.pkl'.format(c)), 'rb') as f:
            assert_same_cov(pickle.load(f), OrderedDict((g, all_cov[g]) for g in z['pkl_{0}_genes'.format(c)].tolist()))
    ref = GeneNMFOA(degnorm_iter=ITER, nmf_iter=NMF_ITER)
    ref.run(cov_e, reads_dat=counts_e[samples].values.astype(np.float64))
    di = pd.read_csv(os.path.join(out, RESULT_FILES[0]))
    assert di.gene.tolist() == list(cov_e) and di.columns.tolist() == ['chr', 'gene'] + samples
    np.testing.assert_allclose(di[samples].values, ref.rho, rtol=1e-12, atol=0)              # the CSV's decimal round trip
    assert all(os.path.isfile(os.path.join(out, name)) for name in RESULT_FILES)
