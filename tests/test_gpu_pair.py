"""
GPU tests of mate pairing on the device (csrc/dn_pair.hip): DeviceRows.pair against numpy on the store's own keys -- order ==
np.argsort(keys, kind='stable'), pair_id == the count of key changes before each position, element for element -- and
NativeBamReadsProcessor(pair='device') against the host path under a stable tie order, run to run, on keys that occur once and
three times, on a hand-made pair whose result depends on the mate order, and through the command line.
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
import _pair_cases as pc                                       # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_bam import _files, _layout_case, _run, _same     # noqa: E402
from degnorm_amd import bam                                    # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure   # noqa: E402
from degnorm_amd.reads import Annotation                       # noqa: E402

pytestmark = pytest.mark.gpu

CHROM = ('c', 1 << 20)


def stable_pair_order(keys):
    """bam.pair_order with equal keys left in file order: what sort_values(kind='stable') would give the reference."""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind='stable').astype(np.int32)
    sk = keys[order]
    pair_id = np.zeros(len(sk), dtype=np.int32)
    if len(sk) > 1:
        np.cumsum(sk[1:] != sk[:-1], out=pair_id[1:])
    return order, pair_id, int(pair_id[-1]) + 1 if len(sk) else 0


def _check_store(rows, n, name):
    keys = rows.keys()
    assert len(keys) == n, name
    order_e, pair_id_e, n_ids_e = pc.oracle(keys)
    order, pair_id, n_ids, ms = rows.pair(fetch=True)
    assert order.dtype == np.int32 and np.array_equal(order, order_e), name
    assert np.array_equal(pair_id, pair_id_e), name
    assert n_ids == n_ids_e and ms >= 0.0, name
    assert rows.pair()[:3] == (None, None, n_ids_e), name
    return keys


def _store_from_file(tmp_path, name, keys, **kw):
    """The keys through a paired BAM file and the reader into a row store (file order = the order of `keys`)."""
    p = str(tmp_path / (name + '.bam'))
    bf.write_bam(p, [CHROM], pc.rows_for(keys))
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / (name + '_out')), verbose=False, **kw)
    proc.paired = True                                         # the store under test, whatever the names say
    return proc, proc.device_rows(CHROM[0])


def test_small_key_sets_equal_numpy(tmp_path):
    """Every ASCII shape of the host test, sizes 0 .. 3 among them, each through a BAM file of its own."""
    for name, keys in pc.key_sets(high=False):
        if not keys:
            rows = bam.DeviceRows(0, True, True)               # no record, no window: the empty store
        else:
            _, rows = _store_from_file(tmp_path, name, keys)
        try:
            got = _check_store(rows, len(keys), name)
            assert [bytes(k) for k in got.tolist()] == keys, name
        finally:
            rows.close()


def test_high_bytes_equal_numpy():
    """Keys with bytes >= 0x80 (the fixture writer takes ASCII names): written over the names of the encoded records."""
    for name, keys in pc.key_sets():
        if name not in ('high_bytes', 'high_random'):
            continue
        keys = [k for k in keys if k and b'.' not in k]
        stand_in = [b'k' * len(k) for k in keys]
        data, offs = bf.encode_records(pc.rows_for(stand_in))
        data = bytearray(data)
        for o, k in zip(offs.tolist(), keys):
            assert bytes(data[o + 36:o + 36 + len(k)]) == b'k' * len(k) and data[o + 36 + len(k)] == ord('.')
            data[o + 36:o + 36 + len(k)] = k
        rows = bam.DeviceRows(0, True, True)
        try:
            rows.append(bytes(data), offs)
            got = _check_store(rows, len(keys), name)
            assert [bytes(k) for k in got.tolist()] == keys and max(max(k) for k in keys) >= 0x80
        finally:
            rows.close()


@pytest.mark.parametrize('n', [64, 65, 70001])
def test_sizes_around_a_wavefront_and_many_workgroups(n, tmp_path):
    """64 and 65 rows; 70 001 rows are more than one workgroup of the hipcub sort and, at 256 lanes, 274 blocks of the kernels."""
    keys = pc.random_keys(n, max(n // 3, 1), seed=n)
    _, rows = _store_from_file(tmp_path, 'n{0}'.format(n), keys)
    try:
        got = _check_store(rows, n, n)
        assert len(set(got.tolist())) > n // 5
    finally:
        rows.close()


@pytest.mark.parametrize('head', [b'p', b'shared--'])
def test_partial_last_chunk_in_more_than_one_block(head, tmp_path):
    """
    5 000 keys whose longest leaves the last chunk partly empty (5 and 12 bytes), so that the pass over it sorts fewer than 64
    bits, in a size for which the radix sort merges blocks (above 1 024 rows); with the 8 shared bytes only that pass tells
    the keys apart.
    """
    rng = np.random.default_rng(4)
    keys = [head + str(i).encode() for i in rng.integers(0, 3000, 5000)]
    _, rows = _store_from_file(tmp_path, 'partial', keys)
    try:
        got = _check_store(rows, len(keys), head)
        assert rows.info()[3] == len(head) + 4 and len(set(got.tolist())) > 2000
    finally:
        rows.close()


def test_ties_follow_file_order_across_windows(tmp_path):
    """A store appended in several windows: equal keys keep the order of the file, not that of a window."""
    keys = pc.random_keys(3000, 600, seed=3, max_len=12)
    for inflate, frame in (('host', 'host'), ('device', 'device')):
        proc, rows = _store_from_file(tmp_path, 'win_' + inflate, keys, window_bytes=20000, inflate=inflate, frame=frame)
        try:
            assert len(list(proc._batches(CHROM[0]))) > 2
            got = _check_store(rows, len(keys), inflate)
            assert [bytes(k) for k in got.tolist()] == keys
        finally:
            rows.close()


@pytest.fixture(scope='module')
def pairs_file(tmp_path_factory):
    """A few thousand synthetic pairs (mates that overlap, contain each other, are swapped or orphaned) as a paired BAM."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(31, 3000, True)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values, 'next_ref': 0})
    p = str(tmp_path_factory.mktemp('pairs') / 'pairs.bam')
    written, _, _ = bf.write_bam(p, [(chrom, chrom_len)], df, straddle=True)
    return p, chrom, ov, gene_df, exon_df, written


@pytest.mark.parametrize('mode', ['host', 'device'])
def test_device_pairing_equals_host_path_with_stable_ties(mode, pairs_file, tmp_path, monkeypatch):
    p, chrom, ov, gene_df, exon_df, written = pairs_file
    n_pairs, n_overlap, _ = pc.order_sensitive_pairs(written.qname.tolist(), written.pos.tolist(), written.cigar.tolist())
    assert n_pairs > 2500 and n_overlap > 500                  # the file has what the tie order matters to
    kw = dict(inflate=mode, frame=mode)
    proc, dev = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'device', pair='device', **kw)
    assert proc.paired and proc.timing['pair_device_ms'] > 0
    monkeypatch.setattr(bam, 'pair_order', stable_pair_order)
    host_proc, host = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'host', pair='host', **kw)
    assert 'pair_device_ms' not in host_proc.timing
    _same(dev, host)
    assert int(dev[2].iloc[:, 1].sum()) > 500


def test_device_pairing_run_to_run(pairs_file, tmp_path):
    p, chrom, ov, gene_df, exon_df, _ = pairs_file
    _, a = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'a', pair='device', inflate='device', frame='device')
    _, b = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'b', pair='device', inflate='device', frame='device')
    _same(a, b)
    for name in sorted(os.listdir(str(tmp_path / 'a'))):
        for f in sorted(os.listdir(str(tmp_path / 'a' / name))):
            if f.endswith('.npz'):
                continue                                       # a zip archive: it holds the time it was written
            with open(str(tmp_path / 'a' / name / f), 'rb') as fa, open(str(tmp_path / 'b' / name / f), 'rb') as fb:
                assert fa.read() == fb.read(), f


def _two_gene_case():
    genes = [('X', [(101, 400)]), ('Y', [(1001, 1300)])]
    gene_df, exon_df = rf.tables('c', genes)
    return 2000, gene_df, exon_df, get_gene_overlap_structure(gene_df)


def test_names_that_occur_once_and_three_times_are_dropped(tmp_path):
    """Pairs on gene X whose mates do not overlap; a name with three reads and a name with one read on gene Y, which must count nothing."""
    chrom_len, gene_df, exon_df, ov = _two_gene_case()
    rows = []
    for i in range(40):
        rows += [('p{0}.1'.format(i), 110 + 2 * i, '20M'), ('p{0}.2'.format(i), 250 + i, '25M')]
    # the third read of t is a second t.1: a suffix 3 would make the reader take the file for single-end
    rows += [('t.1', 1010, '20M'), ('t.2', 1050, '20M'), ('t.1', 1100, '20M'), ('o.1', 1150, '20M'), ('t2.1', 1180, '10M'), ('t2.2', 1200, '10M')]
    df = pd.DataFrame(rows, columns=['qname', 'pos', 'cigar']).assign(ref=0, next_ref=0)
    p = str(tmp_path / 'm.bam')
    bf.write_bam(p, [('c', chrom_len)], df)
    proc, dev = _run(p, 'c', ov, gene_df, exon_df, tmp_path / 'device', pair='device')
    _, host = _run(p, 'c', ov, gene_df, exon_df, tmp_path / 'host', pair='host')
    assert proc.paired
    _same(dev, host)
    counts = dict(zip(dev[2].gene, dev[2].iloc[:, 1].astype(int)))
    assert counts == {'X': 40, 'Y': 1}                          # of Y's reads only the pair t2 counts
    cov = dev[0].toarray().ravel()
    assert cov[1000:1180].sum() == 0 and cov[1180:1190].tolist() == [1] * 10 and cov[1200:1210].tolist() == [1] * 10


def test_mate_inside_its_mate_follows_file_order(tmp_path):
    """
    Read A = [150, 179] comes first in the file, its mate B = [155, 164] lies strictly inside it.  With (A, B), the order of
    the file, the reference's clipping (reads.py:463-467) sends both bounds of B to min(A) - 1 = 149: the pair covers
    [149, 149] and [150, 179], one read on gene X.  (The order (B, A) would clip A to [165, 179] and cover [155, 179].)
    """
    chrom_len, gene_df, exon_df, ov = _two_gene_case()
    df = pd.DataFrame([('m.2', 150, '30M'), ('m.1', 155, '10M')], columns=['qname', 'pos', 'cigar']).assign(ref=0, next_ref=0)
    p = str(tmp_path / 'inside.bam')
    bf.write_bam(p, [('c', chrom_len)], df)
    proc, (csr, ol, cnt) = _run(p, 'c', ov, gene_df, exon_df, tmp_path / 'device', pair='device')
    assert proc.paired
    expect = np.zeros(chrom_len, dtype=np.int64)
    expect[149:180] = 1
    assert np.array_equal(csr.toarray().ravel(), expect)
    assert dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int))) == {'X': 1, 'Y': 0}


def test_argument_checks(tmp_path, monkeypatch):
    single = bam.DeviceRows(0, True, False)
    try:
        with pytest.raises(ValueError, match='dn_bam_rows_pair'):
            single.pair()
    finally:
        single.close()
    chrom_len, gene_df, exon_df, ov = _two_gene_case()
    ann = Annotation(chrom_len, ov, gene_df, exon_df)
    df = pd.DataFrame([('a.1', 110, '20M'), ('a.2', 200, '20M'), ('b.1', 120, '20M'), ('b.2', 220, '20M')],
                      columns=['qname', 'pos', 'cigar']).assign(ref=0, next_ref=0)
    data, offs = bf.encode_records(bf.sort_reads(df))
    rows = bam.DeviceRows(0, True, True)
    try:
        rows.append(data, offs)
        monkeypatch.setattr(bam, 'pair_order', lambda keys: (None, None, 0))       # neither host arrays ...
        with pytest.raises(ValueError, match='dn_bam_rows_coverage: bad argument'):   # ... nor a pairing: as before
            rows.coverage(ann)
        counts = rows.coverage(ann, 'device')[0]
        assert counts.tolist() == [2, 0]
        assert rows.coverage(ann)[0].tolist() == [2, 0]         # null arrays after pair(): the resident pairing
        rows.append(data, offs)                                 # rows appended: the pairing is gone
        with pytest.raises(ValueError, match='dn_bam_rows_coverage: bad argument'):
            rows.coverage(ann)
        assert rows.coverage(ann, 'device')[0].tolist() == [0, 0]       # every name now occurs four times
        with pytest.raises(ValueError, match="pair must be 'host' or 'device', not 'x'"):
            rows.coverage(ann, 'x')
    finally:
        rows.close()


def test_command_with_device_pair_equals_golden(tmp_path):
    """
    python -m degnorm_amd --device-pair --device-inflate --device-frame on the three pipeline samples, in a fresh process.
    Whether the golden is the right expectation is established first, on the host, from the samples' names and positions:
    the samples are single-end (no name ends in .1 / .2 after a '.'), pc.order_sensitive_pairs finds no pair at all in them,
    so none whose mates overlap and none that the stable and the quicksort order treat differently (0 of 0, asserted
    below) -- the flag has nothing to change, and the result must be the pipeline golden.
    """
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    paths, differ = [], 0
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.bam'))
        written, _, _ = bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1), level=6 if k == 2 else 1)
        for tid in range(len(gf.PIPELINE_REFS)):
            w = written[written.ref == tid]
            n_pairs, n_overlap, n_differ = pc.order_sensitive_pairs(w.qname.tolist(), w.pos.tolist(), w.cigar.tolist())
            print('sample {0} ref {1}: {2} pairs, {3} with overlapping mates, {4} ordered differently'.format(s, tid, n_pairs, n_overlap, n_differ))
            differ += n_differ
        paths.append(p)
    assert differ == 0
    z = golden('pipeline')
    minimax = int(z['case_a_minimax'])
    all_cov, _, all_counts, _ = golden_inputs(z, [])
    out = str(tmp_path / 'out')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--device-pair', '--device-inflate', '--device-frame', '--bam-files'] + paths + \
          ['--bai-files'] + [p + '.bai' for p in paths] + ['-g', GTF, '-o', out, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER),
                                                           '--minimax-coverage', str(minimax)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'gene_exon_metadata.csv')), golden_frame(z, 'exon', RUN_COLS).reset_index(drop=True))
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'read_counts.csv')), all_counts)
    for c in z['chroms'].tolist():
        with open(os.path.join(out, c, 'coverage_matrices_{0}.pkl'.format(c)), 'rb') as f:
            assert_same_cov(pickle.load(f), OrderedDict((g, all_cov[g]) for g in z['pkl_{0}_genes'.format(c)].tolist()))
    assert all(os.path.isfile(os.path.join(out, name)) for name in RESULT_FILES)
