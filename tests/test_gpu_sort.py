"""
GPU tests of the coordinate sort of BAM files on the device (csrc/dn_sort.hip, degnorm_amd.bam.sort_bam(device=0)): the cases,
window and segment sizes of tests/_sort_cases.py against the host build file for file (which tests/test_sort_host.py holds
against the definition in plain Python); the refused files (sent to the device only after the valid cases have passed in this
run and the host build has given the expected text); the memory check; and `python -m degnorm_amd --sort-bam` on the pipeline
samples written unsorted and without index against tests/golden/pipeline.npz.
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
import _sort_cases as sc                                       # noqa: E402
from conftest import golden                                    # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = set()                                          # the cases whose device output equalled the host's in this run


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_device_sort_equals_host_sort(name, tmp_path):
    src = str(tmp_path / 'in.bam')
    case = sc.build_case(name, src)
    host, dev = str(tmp_path / 'host.bam'), str(tmp_path / 'dev.bam')
    bam.sort_bam(src, host)
    expect = open(host, 'rb').read()
    assert sc.inflate_file(host)[0] == case['header_out'] + sc.spec_sorted(case['stream'])[0]
    for window_bytes in sc.WINDOWS:
        for segment_bytes in sc.SEGMENTS:
            stats = {}
            bam.sort_bam(src, dev, device=0, window_bytes=window_bytes, segment_bytes=segment_bytes, overwrite=True, stats=stats)
            assert open(dev, 'rb').read() == expect, (name, window_bytes, segment_bytes)
            assert stats['records'] == len(case['rows']) and stats['bytes'] == len(case['stream']) and stats['frame_fixups'] >= 0
            if len(case['rows']):
                assert stats['inflate_device_ms'] > 0 and stats['frame_device_ms'] > 0
                assert stats['sort_device_ms'] > 0 and stats['gather_device_ms'] > 0
            assert stats['windows'] == 1 if window_bytes is None else stats['windows'] >= 1
    _VALID_PASSED.add(name)


def test_errors_equal_the_host_texts(tmp_path):
    assert len(_VALID_PASSED) == len(sc.CASES), 'no error input goes to the device before the valid cases have passed in this run'
    for name, (path, kw, text) in sc.error_files(tmp_path).items():
        for sizes in ({}, {'window_bytes': 1, 'segment_bytes': 256}):
            dst = str(tmp_path / (name + '_out.bam'))
            with pytest.raises(ValueError) as host:
                bam.sort_bam(path, dst, **dict(kw, **sizes))
            assert text in str(host.value), name                   # the host build first
            with pytest.raises(ValueError) as dev:
                bam.sort_bam(path, dst, device=0, **dict(kw, **sizes))
            assert str(dev.value) == str(host.value), (name, sizes)
            assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')
    # a valid call after an error works
    src = str(tmp_path / 'ok.bam')
    sc.build_case('three', src)
    a, b = str(tmp_path / 'a.bam'), str(tmp_path / 'b.bam')
    assert open(bam.sort_bam(src, a, device=0), 'rb').read() == open(bam.sort_bam(src, b), 'rb').read()


def test_memory_check_comes_before_any_upload(tmp_path):
    src = str(tmp_path / 'in.bam')
    case = sc.build_case('three', src)
    dst = str(tmp_path / 'out.bam')
    free, total = bam.device_memory(0)
    assert 0 < free <= total
    with pytest.raises(ValueError) as e:
        bam.sort_bam(src, dst, device=0, max_device_bytes=len(case['stream']))
    assert 'bytes of device memory' in str(e.value) and '{0} are allowed'.format(len(case['stream'])) in str(e.value)
    assert '({0} bytes of records)'.format(len(case['stream'])) in str(e.value) and src in str(e.value)
    assert not os.path.exists(dst) and not os.path.exists(dst + '.tmp')
    assert bam.sort_bam(src, dst, device=0, max_device_bytes=64 << 20) == dst


def _unsorted_copy(path, refs, rows, seed, straddle):
    """
    Write the sorted fixture's records in a seeded order that keeps records of equal (refID, pos) in their relative order,
    with SO:unsorted and without index.  Returns the inflated bytes of the sorted fixture (header and records).
    """
    rows = bf.sort_reads(rows)
    data, offs = bf.encode_records(rows)
    ends = np.append(offs[1:], len(data))
    perm = np.random.default_rng(seed).permutation(len(rows))
    group = rows.groupby(['ref', 'pos'], sort=False).ngroup().values
    where = np.argsort(perm, kind='stable')                    # where[k]: the place record k goes to
    for g in np.flatnonzero(np.bincount(group) > 1):
        members = np.flatnonzero(group == g)
        where[members] = np.sort(where[members])               # members in ascending order of original index, on their places
    order = np.argsort(where, kind='stable')
    assert sorted(order.tolist()) == list(range(len(rows))) and (order != np.arange(len(rows))).any()
    shuffled = b''.join(data[offs[k]:ends[k]] for k in order.tolist())
    new_offs = np.concatenate([[0], np.cumsum((ends - offs)[order])[:-1]])
    hdr = bf.header_bytes(refs, text='@HD\tVN:1.6\tSO:unsorted\n')
    bc.write_layout(path, hdr, shuffled, bc.layout_cuts('straddle' if straddle else 'aligned', len(hdr), new_offs, len(shuffled)), 1)
    return bf.header_bytes(refs) + data


def test_command_sorts_unsorted_inputs_and_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.nmf import GeneNMFOA
    paths, fixtures = [], []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.bam'))
        fixtures.append(_unsorted_copy(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), 40 + k, straddle=(k == 1)))
        paths.append(p)
        assert bam.sort_order(p) == 'unsorted'
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    all_cov, _, all_counts, _ = golden_inputs(z, [])
    out = str(tmp_path / 'out')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--sort-bam', '--device-inflate', '--device-frame', '--bam-files'] + paths + \
          ['-g', GTF, '-o', out, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)]
    # with --create-bai in place of --sort-bam the command stops at the first record out of order
    r = subprocess.run(['--create-bai' if c == '--sort-bam' else c for c in cmd], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=600)
    assert r.returncode != 0 and 'not sorted by coordinate' in r.stdout and not os.path.exists(out)
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith('.bai')]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    # the sorted copies are kept, are the sorted fixtures byte for byte, and are indexed there; nothing is written beside the inputs
    assert sorted(os.listdir(os.path.join(out, 'sorted_bam'))) == sorted(s + e for s in gf.PIPELINE_SAMPLES for e in ('.bai', '.bam'))
    assert sorted(os.listdir(str(tmp_path))) == sorted([s + '.bam' for s in gf.PIPELINE_SAMPLES] + ['out'])
    for s, expect in zip(gf.PIPELINE_SAMPLES, fixtures):
        p = os.path.join(out, 'sorted_bam', s + '.bam')
        assert sc.inflate_file(p)[0] == expect
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
