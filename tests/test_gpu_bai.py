"""
GPU tests of .bai creation on the device (csrc/dn_bai.hip, degnorm_amd.bam.build_index(device=0)): the cases, layouts, window
and segment sizes of tests/_bai_cases.py against the host build byte for byte (which tests/test_bai_host.py holds against the
pure-Python specification); the reader on a created index against the reader on the fixture writer's index; the error files
(sent to the device only after the valid cases have passed in this run and the host build has given the expected text); and
`python -m degnorm_amd --create-bai` on the pipeline samples without their indexes against tests/golden/pipeline.npz.
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
from conftest import golden                                    # noqa: E402
from test_gpu_reads import _case                               # noqa: E402
from test_gpu_bam import _run, _same                           # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = set()                                          # (case, layout) whose device index equalled the host's in this run


@pytest.mark.parametrize('layout', bc.LAYOUTS)
@pytest.mark.parametrize('name', sorted(bc.CASES))
def test_device_build_equals_host_build(name, layout, tmp_path):
    p = str(tmp_path / 'c.bam')
    refs, records, blocks, reads = bc.build_case(name, layout, p, level=6 if layout == 'empty' else 1)
    expect = bam.build_index(p).tobytes()
    assert len(expect) > 1000
    for window_bytes in bc.WINDOWS:
        for segment_bytes in bc.SEGMENTS:
            stats = {}
            got = bam.build_index(p, device=0, window_bytes=window_bytes, segment_bytes=segment_bytes, stats=stats)
            assert got.tobytes() == expect, (name, layout, window_bytes, segment_bytes)
            assert stats['index_device_ms'] > 0 and stats['inflate_device_ms'] > 0 and stats['frame_device_ms'] > 0
            assert stats['records'] == len(reads) and stats['chunks'] > 0 and stats['frame_fixups'] >= 0
            assert stats['windows'] == 1 if window_bytes is None else stats['windows'] > (20 if window_bytes == 1 else 3)
    _VALID_PASSED.add((name, layout))


def test_errors_equal_the_host_texts(tmp_path):
    assert len(_VALID_PASSED) == len(bc.CASES) * len(bc.LAYOUTS), 'no error input goes to the device before the valid cases have passed in this run'
    for name, (path, text) in bc.error_files(tmp_path).items():
        for kw in bc.ERROR_SIZES:
            with pytest.raises(ValueError) as host:
                bam.build_index(path, **kw)
            assert text in str(host.value), name                   # the host build first
            with pytest.raises(ValueError) as dev:
                bam.build_index(path, device=0, **kw)
            assert str(dev.value) == str(host.value), (name, kw)
    # a valid call after an error works
    p = str(tmp_path / 'ok.bam')
    bc.build_case('three', 'straddle', p)
    assert bam.build_index(p, device=0).tobytes() == bam.build_index(p).tobytes()


@pytest.mark.parametrize('key', ['se', 'pe'])
def test_reader_on_created_index_equals_reader_on_fixture_index(key, tmp_path):
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
    assert not os.path.exists(ours + '.bai') and bam.create_index(ours, device=0) == ours + '.bai'
    assert bam.parse_bai(ours + '.bai').pseudo(0) == bam.read_bai(theirs + '.bai')[0][0]['pseudo']
    for inflate in ('host', 'device'):
        for frame in ('host', 'device'):
            _, a = _run(theirs, 'c', ov, gene_df, exon_df, tmp_path / 'theirs' / (inflate + frame), inflate=inflate, frame=frame)
            proc, b = _run(ours, 'c', ov, gene_df, exon_df, tmp_path / 'ours' / (inflate + frame), inflate=inflate, frame=frame)
            _same(a, b)
            assert proc.paired == paired and int(b[2].iloc[:, 1].sum()) > 100


def test_command_creates_missing_indexes_and_equals_golden(tmp_path):
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
    cmd = [sys.executable, '-m', 'degnorm_amd', '--create-bai', '--device-inflate', '--device-frame', '--bam-files'] + paths + \
          ['-g', GTF, '-o', out, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)]
    # without the flag the command stops at the missing index
    r = subprocess.run([c for c in cmd if c != '--create-bai'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=600)
    assert r.returncode != 0 and 'No .bai index file' in r.stdout and not os.path.exists(out)
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    for p in paths:
        idx = bam.parse_bai(p[:-3] + 'bai')
        assert idx.tobytes() == bam.build_index(p).tobytes() and len(idx.refs) == len(gf.PIPELINE_REFS)
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.bai')) == sorted(s + '.bai' for s in gf.PIPELINE_SAMPLES)
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
