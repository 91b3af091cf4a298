"""
GPU tests of the SAM encoder on the device (csrc/dn_sam.hip; degnorm_amd.bam.sam_records / sam_to_bam with device=0): the valid
cases of tests/_sam_cases.py against the host build byte for byte (which tests/test_sam_host.py holds against the definition in
plain Python), with every window size and both encoders of the blocks; the malformed inputs (sent to the device only after the
valid cases have passed in this run and the host build has given the expected text); the fixture rows read back by
NativeBamReadsProcessor; and `python -m degnorm_amd --sam-files` on the pipeline samples written as shuffled SAM text against
tests/golden/pipeline.npz.
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

import _bam_fixtures as bf                                     # noqa: E402
import _sam_cases as sc                                        # noqa: E402
import _sort_cases as sortc                                    # noqa: E402
from conftest import golden                                    # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = set()                                          # the cases whose device output equalled the host's in this run


@pytest.mark.parametrize('name', sorted(sc.VALID))
def test_device_records_equal_host_records(name, tmp_path):
    text = sc.VALID[name]
    host_stats, stats = {}, {}
    expect, expect_off = bam.sam_records(text, sc.REFS, stats=host_stats)
    stream, off = bam.sam_records(text, sc.REFS, device=0, stats=stats)
    assert stream == expect and off.tolist() == expect_off.tolist()
    assert {k: stats[k] for k in ('lines', 'records', 'float_patches')} == {k: host_stats[k] for k in ('lines', 'records', 'float_patches')}
    assert (stats['encode_device_ms'] > 0) == (len(text) > 0)
    src, host, dev = sc.write_sam(str(tmp_path / 'in.sam'), text), str(tmp_path / 'host.bam'), str(tmp_path / 'dev.bam')
    for deflate in ('zlib', 'native'):
        for window_bytes in (None, 1, 4096):
            if window_bytes == 1 and name in ('n255', 'n256', 'straddle_tile'):
                continue                                        # one window, and one launch, per line: n257 has that case
            kw = dict({} if window_bytes is None else {'window_bytes': window_bytes}, deflate=deflate, overwrite=True)
            bam.sam_to_bam(src, host, **kw)
            stats = {}
            bam.sam_to_bam(src, dev, device=0, stats=stats, **kw)
            assert open(dev, 'rb').read() == open(host, 'rb').read(), (name, deflate, window_bytes)
            assert stats['records'] == len(off) - 1 and (stats['encode_device_ms'] > 0) == (stats['records'] > 0)
    _VALID_PASSED.add(name)


def test_errors_equal_the_host_texts(tmp_path):
    assert len(_VALID_PASSED) == len(sc.VALID), 'no malformed input goes to the device before the valid cases have passed in this run'
    n_head = sc.HEADER.count('\n')
    for name, (text, line, kind) in sorted(sc.ERRORS.items()):
        with pytest.raises(ValueError) as host:
            bam.sam_records(text, sc.REFS)
        assert str(host.value) == 'line {0}: {1}'.format(line, sc.TEXT[kind]), name           # the host build first
        with pytest.raises(ValueError) as dev:
            bam.sam_records(text, sc.REFS, device=0)
        assert str(dev.value) == str(host.value), name
        src, dst = sc.write_sam(str(tmp_path / (name + '.sam')), text), str(tmp_path / (name + '.bam'))
        for kw in ({}, {'window_bytes': 4096}):
            with pytest.raises(ValueError) as dev:
                bam.sam_to_bam(src, dst, device=0, **kw)
            assert str(dev.value) == '{0}: line {1}: {2}'.format(src, n_head + line, sc.TEXT[kind]), (name, kw)
            assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')
    # a valid call after an error works
    stream, off = bam.sam_records(sc.VALID['tag_f'], sc.REFS, device=0)
    expect, expect_off = bam.sam_records(sc.VALID['tag_f'], sc.REFS)
    assert stream == expect and off.tolist() == expect_off.tolist()


def test_reader_loads_the_same_reads_as_from_the_fixture_bam(tmp_path):
    """The round trip on meaning: the rows of _bam_fixtures as shuffled SAM text, converted, sorted and indexed, give
    NativeBamReadsProcessor the reads it loads from the BAM file the fixture's own writer makes of the same rows."""
    rng = np.random.default_rng(11)
    n = 900
    rows = pd.DataFrame({'ref': rng.choice([0, 1, -1], n, p=[0.6, 0.3, 0.1]), 'pos': rng.integers(0, 90000, n),
                         'qname': ['r{0}'.format(i) for i in range(n)],
                         'cigar': rng.choice(['50M', '20M100N30M', '5S40M5S', '10M2I10M1D18M', '7M'], n),
                         'nh': rng.choice([1, 1, 1, 2], n), 'nh_type': rng.choice(list('cCsSiI'), n)})
    rows.loc[rows.ref < 0, 'pos'] = -1
    fixture = str(tmp_path / 'fixture.bam')
    rows = bf.write_bam(fixture, sc.REFS, rows)[0]
    lines = sc.sam_text(rows, sc.REFS).split(b'\n')[:-1]
    src = sc.write_sam(str(tmp_path / 'x.sam'), b''.join(lines[k] + b'\n' for k in sc.shuffled_order(rows, 4)))
    for device in (None, 0):
        conv = bam.sam_to_bam(src, str(tmp_path / 'x.bam'), device=device, window_bytes=30000, overwrite=True)
        srt = bam.sort_bam(conv, str(tmp_path / 'x_sorted.bam'), device=device, overwrite=True)
        bam.create_index(srt, device=device, overwrite=True)
        for unique in (True, False):
            want = bam.NativeBamReadsProcessor(fixture, fixture + '.bai', unique_alignment=unique, verbose=False)
            got = bam.NativeBamReadsProcessor(srt, srt + '.bai', unique_alignment=unique, verbose=False)
            assert got.paired == want.paired
            for chrom in ('c1', 'c2'):
                pd.testing.assert_frame_equal(got.load_chromosome_reads(chrom), want.load_chromosome_reads(chrom))


def _shuffled_sam(path, refs, rows, seed):
    """The sample's rows as SAM text in a seeded order that keeps rows of equal (refID, pos) in their relative order, under a
    header without SO:.  Returns the inflated bytes the converted file must have, and those of its coordinate-sorted copy."""
    rows = bf.sort_reads(rows)
    lines = sc.sam_text(rows, refs).split(b'\n')[:-1]
    text = b''.join(lines[k] + b'\n' for k in sc.shuffled_order(rows, seed))
    header = '@HD\tVN:1.6\n' + ''.join('@SQ\tSN:{0}\tLN:{1}\n'.format(nm, ln) for nm, ln in refs) + '@PG\tID:aligner\tCL:align a b\n'
    sc.write_sam(path, text, header)
    head = sc.bam_header(header, refs)
    stream = sc.encode(text, refs)[0]
    return head + stream, bam.coordinate_header(head) + sortc.spec_sorted(stream)[0]


def test_command_converts_sam_inputs_and_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.nmf import GeneNMFOA
    paths, expect = [], []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.sam'))
        expect.append(_shuffled_sam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), 40 + k))
        paths.append(p)
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    all_cov, _, all_counts, _ = golden_inputs(z, [])
    out = str(tmp_path / 'out')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--device-inflate', '--device-frame', '--sam-files'] + paths + \
          ['-g', GTF, '-o', out, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    # converted_bam/ holds the records in input order, sorted_bam/ the sorted copies and their indexes; nothing beside the inputs
    assert sorted(os.listdir(os.path.join(out, 'converted_bam'))) == sorted(s + '.bam' for s in gf.PIPELINE_SAMPLES)
    assert sorted(os.listdir(os.path.join(out, 'sorted_bam'))) == sorted(s + e for s in gf.PIPELINE_SAMPLES for e in ('.bai', '.bam'))
    assert sorted(os.listdir(str(tmp_path))) == sorted([s + '.sam' for s in gf.PIPELINE_SAMPLES] + ['out'])
    for s, (converted, sorted_copy) in zip(gf.PIPELINE_SAMPLES, expect):
        assert sortc.inflate_file(os.path.join(out, 'converted_bam', s + '.bam'))[0] == converted
        p = os.path.join(out, 'sorted_bam', s + '.bam')
        assert sortc.inflate_file(p)[0] == sorted_copy
        assert bam.parse_bai(p[:-3] + 'bai').tobytes() == bam.build_index(p).tobytes()
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
