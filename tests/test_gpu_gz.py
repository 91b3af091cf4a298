"""
GPU tests of the gzip inflate (csrc/dn_gz.hip; degnorm_amd.gz with device=0) against the host build of the same source, which
tests/test_gz_host.py holds against Python's gzip and a plain-Python restatement of the definition: the bytes, the guess and
segment tables, every counter and every error text on the cases of tests/_gz_cases.py; streams of 1, 2, 63, 64 and 65 chunks;
spans; and the readers that take .gz files -- the annotation loaders, sam_to_bam and the command.
"""
import gzip
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gz_cases as gc                                         # noqa: E402
from degnorm_amd import bam, gz, loaders                       # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(gc.cases())
COUNTERS = ('members', 'chunks', 'guessed', 'confirmed', 'jumped', 'fixups', 'segments', 'blocks', 'bytes_in', 'bytes_out', 'bgzf')


def _same_as_host(z, chunk, window=None):
    host, dev = {}, {}
    want = gz.gunzip(z, chunk_bytes=chunk, window_bytes=window, stats=host)
    got = gz.gunzip(z, device=0, chunk_bytes=chunk, window_bytes=window, stats=dev)
    assert got == want
    assert {k: dev[k] for k in COUNTERS} == {k: host[k] for k in COUNTERS}
    assert all(dev[k] >= 0.0 for k in gz.STAGES)
    return want, dev


@pytest.mark.parametrize('name', NAMES)
def test_device_equals_host(name):
    z, plain = gc.cases()[name]
    for chunk in (4096, 65536):
        want, _ = _same_as_host(z, chunk)
        assert want == plain
        guess_h, seg_h = gz.scan(z, chunk_bytes=chunk)
        guess_d, seg_d = gz.scan(z, device=0, chunk_bytes=chunk)
        np.testing.assert_array_equal(guess_d, guess_h)
        np.testing.assert_array_equal(seg_d, seg_h)


@pytest.fixture(scope='module')
def long_stream():
    """A level-6 text case of more than 65 chunks of 4 KiB (the cases of _gz_cases.py are sized for the restatement)."""
    text = gc.gtf_text(9500000, seed=25)
    z = gc.member(text, 6)
    assert len(z) > 65 * 4096
    return z, text


def member_of_chunks(text, n_chunks):
    """A level-6 member of a prefix of text, padded with zero bytes (which a reader ignores) to exactly n_chunks chunks of 4 KiB."""
    lo, hi = 0, len(text)
    while True:                                                   # the compressed size grows with the prefix: bisect it
        mid = (lo + hi) // 2
        m = gc.member(text[:mid], 6)
        if len(m) > n_chunks * 4096:
            hi = mid
        elif len(m) <= (n_chunks - 1) * 4096:
            lo = mid
        else:
            return m + b'\0' * (n_chunks * 4096 - len(m)), text[:mid]


@pytest.mark.parametrize('n_chunks', [1, 2, 63, 64, 65])
def test_streams_of_n_chunks(long_stream, n_chunks):
    """Files of exactly n chunks of 4 KiB: 64 fill a step of 64 workgroups exactly, 65 overflow it by one.  Then the stream cut
    behind n chunks: an error behind the segments that precede the cut, with the host's text."""
    z, text = long_stream
    data, plain = member_of_chunks(text, n_chunks)
    want, st = _same_as_host(data, 4096)
    assert want == plain and st['chunks'] == n_chunks
    guess_h, seg_h = gz.scan(data, chunk_bytes=4096)
    guess_d, seg_d = gz.scan(data, device=0, chunk_bytes=4096)
    np.testing.assert_array_equal(guess_d, guess_h)
    np.testing.assert_array_equal(seg_d, seg_h)
    with pytest.raises(ValueError) as dev:
        gz.gunzip(z[:n_chunks * 4096], device=0, chunk_bytes=4096)
    assert str(dev.value) == '<bytes>: gzip member at byte 0: truncated deflate stream'


def test_whole_long_stream(long_stream):
    z, text = long_stream
    want, st = _same_as_host(z, 4096)
    assert want == text and st['confirmed'] > 1                  # beyond the member's first block: a blind walk joined the chain
    want, st = _same_as_host(z, 65536)
    assert want == text


@pytest.mark.parametrize('name', ['text6', 'run', 'sync_flush', 'three_members', 'nested'])
def test_spans_equal_one_span(name):
    z, plain = gc.cases()[name]
    want, _ = _same_as_host(z, 4096, window=65536)
    assert want == plain


@pytest.fixture(scope='module')
def valid_cases_pass():
    """No malformed input goes to the device before the valid cases have given the host's bytes there, in this run and in
    whatever order or selection the tests are run."""
    for name in NAMES:
        _same_as_host(gc.cases()[name][0], 4096)


def test_errors_equal_the_host_texts(valid_cases_pass):
    for name, data, offset, what in gc.error_cases():
        for chunk in (4096, 65536):
            with pytest.raises(ValueError) as dev:
                gz.gunzip(data, device=0, chunk_bytes=chunk)
            assert str(dev.value) == '<bytes>: gzip member at byte {0}: {1}'.format(offset, what), name
    z, plain = gc.cases()['one_byte']
    assert gz.gunzip(z, device=0) == plain                         # a valid call after an error works


def test_bgzf_takes_the_block_path():
    text = gc.cases()['text6'][1][:300000]
    z = b''.join(bam.bgzf_compress(text[lo:lo + 0xff00], 6) for lo in range(0, len(text), 0xff00)) + bam.BGZF_EOF
    st = {}
    assert gz.gunzip(z, device=0, stats=st) == text and st['bgzf'] is True


def _gz_copy(path):
    with open(path, 'rb') as f:
        data = f.read()
    with open(path + '.gz', 'wb') as f:
        f.write(gzip.compress(data, 6))
    return path + '.gz'


def test_annotation_loaders_take_gz(tmp_path):
    import _gff3_fixtures as g3
    import _gtf_fixtures as gf
    gtf = str(tmp_path / 'x.gtf')
    gf.write_gtf(gtf, 31, 200000)
    want = loaders.annotation_loader(gtf, window_bytes=4096, device=0).get_data()
    got = loaders.annotation_loader(_gz_copy(gtf), window_bytes=4096, device=0).get_data()
    pd.testing.assert_frame_equal(got, want)
    for dialect in g3.DIALECTS:
        _, gff3 = g3.write_twin(str(tmp_path), 32, 200000, dialect)[:2]
        want = loaders.annotation_loader(gff3, window_bytes=4096, device=0).get_data()
        got = loaders.annotation_loader(_gz_copy(gff3), window_bytes=4096, device=0).get_data()
        pd.testing.assert_frame_equal(got, want)


def test_sam_to_bam_takes_gz(tmp_path):
    import _sam_cases as sc
    text = b''.join(sc.VALID[k] for k in sorted(sc.VALID) if sc.VALID[k].endswith(b'\n'))
    src = sc.write_sam(str(tmp_path / 'x.sam'), text)
    plain = bam.sam_to_bam(src, str(tmp_path / 'plain.bam'), device=0)
    zipped = bam.sam_to_bam(_gz_copy(src), str(tmp_path / 'zipped.bam'), device=0)
    assert open(zipped, 'rb').read() == open(plain, 'rb').read()


def test_command_takes_gz_inputs_and_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from conftest import golden
    from test_annotation_host import RUN_COLS, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, golden_inputs
    from test_gpu_sam import _shuffled_sam
    from degnorm_amd.nmf import GeneNMFOA
    paths = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.sam'))
        _shuffled_sam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), 40 + k)
        paths.append(_gz_copy(p))
        os.remove(p)
    genes = str(tmp_path / 'genes.gtf')
    with open(GTF, 'rb') as f, open(genes, 'wb') as g:
        g.write(f.read())
    genes_gz = _gz_copy(genes)
    os.remove(genes)
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    _, _, all_counts, _ = golden_inputs(z, [])
    out = str(tmp_path / 'out')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--device-inflate', '--device-frame', '--sam-files'] + paths + \
          ['-g', genes_gz, '-o', out, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert sorted(os.listdir(os.path.join(out, 'converted_bam'))) == sorted(s + '.bam' for s in gf.PIPELINE_SAMPLES)
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'gene_exon_metadata.csv')), golden_frame(z, 'exon', RUN_COLS).reset_index(drop=True))
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out, 'read_counts.csv')), all_counts)
    ref = GeneNMFOA(degnorm_iter=ITER, nmf_iter=NMF_ITER)
    ref.run(cov_e, reads_dat=counts_e[samples].values.astype(np.float64))
    di = pd.read_csv(os.path.join(out, RESULT_FILES[0]))
    assert di.gene.tolist() == list(cov_e) and di.columns.tolist() == ['chr', 'gene'] + samples
    np.testing.assert_allclose(di[samples].values, ref.rho, rtol=1e-12, atol=0)              # the CSV's decimal round trip


def test_run_pipeline_takes_gtf_gz(tmp_path):
    import _bam_fixtures as bf
    import _gtf_fixtures as gf
    from conftest import golden
    from test_annotation_host import RUN_COLS, assert_same_table, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, assert_same_cov, golden_inputs
    from degnorm_amd.pipeline import run_pipeline
    bam_files = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.bam'))
        bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1))
        bam_files.append(p)
    genes = str(tmp_path / 'genes.gtf')
    with open(GTF, 'rb') as f, open(genes, 'wb') as g:
        g.write(f.read())
    genes_gz = _gz_copy(genes)
    os.remove(genes)
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    out = str(tmp_path / 'out')
    os.makedirs(out)
    _, _, cov, counts_df, genes_df, exon_df, sample_ids = run_pipeline(
        bam_files, [p + '.bai' for p in bam_files], genes_gz, out, degnorm_iter=ITER, nmf_iter=NMF_ITER, minimax_coverage=minimax, verbose=False)
    assert sample_ids == samples
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_cov(cov, cov_e)
