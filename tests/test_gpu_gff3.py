"""
GPU tests of the GFF3 scan on the device (csrc/dn_gff3.hip; loaders.gff3_scan with device=0, Gff3AnnotationLoader): every
text of tests/_gff3_fixtures.py against the host build (which tests/test_gff3_host.py holds against the restatement in plain
Python, and which walks every text here before the device sees it), the loader with 4 KiB windows against one window, a
16 MB twin per dialect against the GTF loader on the GTF twin, and the pipeline with a GFF3 annotation against
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

import _gff3_fixtures as g3                                            # noqa: E402
import _gtf_fixtures as gf                                             # noqa: E402
from conftest import golden                                            # noqa: E402
from test_gff3_host import scan_rows                                   # noqa: E402
from degnorm_amd import _lib, loaders                                  # noqa: E402
from degnorm_amd.gene_processing import GeneAnnotationProcessor        # noqa: E402
from degnorm_amd.loaders import GeneAnnotationLoader, Gff3AnnotationLoader     # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = set()                                          # the texts whose device rows equalled the host's in this run


def table_of(outcome):
    return pd.DataFrame({'chr': np.array([r[1].decode() for r in outcome[2]], dtype=object), 'start': np.array([r[2] for r in outcome[2]], dtype=np.int64),
                         'end': np.array([r[3] for r in outcome[2]], dtype=np.int64),
                         'gene': np.array([r[4].decode() for r in outcome[2]], dtype=object)}).drop_duplicates().reset_index(drop=True)


@pytest.mark.parametrize('name', sorted(g3.CASES))
def test_device_rows_equal_host_rows(name):
    data = g3.CASES[name]
    for bits in (64, 4):
        host_stats, stats = {}, {}
        want = g3.outcome(scan_rows, data, hash_bits=bits, stats=host_stats)            # the host build first
        assert want[0] == 'rows'
        assert g3.outcome(scan_rows, data, device=0, hash_bits=bits, stats=stats) == want, (name, bits)
        assert stats == host_stats
    _VALID_PASSED.add(name)


def test_device_errors_equal_host_errors(tmp_path):
    assert len(_VALID_PASSED) == len(g3.CASES), 'no malformed input goes to the device before the valid texts have passed in this run'
    for name, (data, line, kind) in sorted(g3.ERRORS.items()):
        for bits in (64, 4):
            assert g3.outcome(scan_rows, data, hash_bits=bits) == ('error', line, kind), name
            assert g3.outcome(scan_rows, data, device=0, hash_bits=bits) == ('error', line, kind), (name, bits)
        # a damaged file through the loader: the file, the line and the kind, whatever the windows
        p = tmp_path / (name + '.gff3')
        p.write_bytes(data)
        for window_bytes in (None, 64):
            with pytest.raises(ValueError) as e:
                Gff3AnnotationLoader(str(p), window_bytes=window_bytes).get_data()
            assert str(e.value) == 'File {0}, line {1} {2}'.format(p, line, g3.TEXT[kind]), (name, window_bytes)
    # a valid call after an error works
    assert g3.outcome(scan_rows, g3.CASES['ensembl_small'], device=0) == g3.outcome(scan_rows, g3.CASES['ensembl_small'])


def test_mutations_on_the_device_equal_the_host_build():
    assert len(_VALID_PASSED) == len(g3.CASES)
    for data in g3.mutations(150, seed=9):
        assert g3.outcome(scan_rows, data, device=0) == g3.outcome(scan_rows, data), data


def test_a_file_that_does_not_fit_is_refused_before_anything_is_uploaded():
    with pytest.raises(ValueError, match='needs about .* MiB of device memory'):
        loaders.Gff3Scan(1 << 50, device=0)
    with loaders.Gff3Scan(100, device=0) as scan:
        with pytest.raises(ValueError, match='more bytes than the handle was opened for'):
            scan.window(b'x' * 101)
        cols, err, _, _ = scan.window(g3.CASES['one_line_newline'])
        assert err is None and cols['line'].tolist() == [1] and cols['pending'].tolist() == [0]
        with pytest.raises(ValueError, match='outside the bytes uploaded'):
            scan.resolve(np.array([1]), np.array([90]), np.array([40]), np.array([0], dtype=np.uint64))


@pytest.mark.parametrize('name', sorted(g3.CASES))
def test_small_windows_give_the_single_window_table(name, tmp_path):
    p = tmp_path / 'x.gff3'
    p.write_bytes(g3.CASES[name])
    want = table_of(g3.outcome(scan_rows, g3.CASES[name]))
    for window_bytes in (None, 1, 100, 4096):
        pd.testing.assert_frame_equal(Gff3AnnotationLoader(str(p), window_bytes=window_bytes).get_data(), want)


def test_loader_with_4k_windows_equals_one_window(tmp_path):
    """About 300 KB in the ensembl dialect: parents and children in different windows, a line longer than a window, windows
    that start and end inside a 16 KiB tile."""
    _, path = g3.write_twin(str(tmp_path), 8, 600000, 'ensembl')
    lines = open(path, 'rb').read().split(b'\n')
    lines.insert(len(lines) // 2, g3._LONG.replace(b'ID=transcript:T2;Parent=gene:G1', b'ID=long;Parent=gene:ENSG00000000000.1'))
    lines.insert(5, g3._ln('c9', 'exon', 1, 2, 'Parent=long'))
    data = b'\n'.join(lines)
    with open(path, 'wb') as f:
        f.write(data)
    host_stats = {}
    want = g3.outcome(scan_rows, data, stats=host_stats)
    assert want == g3.outcome(g3.restate, data) and want[2][0][4] == b'GENE0'
    one = Gff3AnnotationLoader(path)
    pd.testing.assert_frame_equal(one.get_data(), table_of(want))
    small = Gff3AnnotationLoader(path, window_bytes=4096)
    first = small.get_data()
    pd.testing.assert_frame_equal(first, table_of(want))
    assert isinstance(first.index, pd.RangeIndex) and [str(t) for t in first.dtypes] == ['object', 'int64', 'int64', 'object']
    t = small.timing
    assert t['bytes'] == len(data) and t['lines'] == want[1] == one.timing['lines'] and t['walked_exons'] == len(want[2])
    assert t['nodes'] == one.timing['nodes'] == host_stats['nodes'] > 100 and t['resolve_ms'] > 0 and t['device_ms'] > 0
    pd.testing.assert_frame_equal(Gff3AnnotationLoader(path, window_bytes=4096).get_data(), first)          # two runs are identical
    # the same text with sequence behind it: the loader stops at ##FASTA
    with open(path, 'ab') as f:
        f.write(b'\n##FASTA\n>c1\n' + b'ACGT' * 5000 + b'\n')
    tail = Gff3AnnotationLoader(path, window_bytes=4096)
    pd.testing.assert_frame_equal(tail.get_data(), first)
    assert tail.timing['bytes'] < len(data) + 4096 + 20


@pytest.mark.parametrize('dialect', g3.DIALECTS)
def test_twin_files_give_the_table_of_the_gtf_loader(dialect, tmp_path):
    gtf, gff3 = g3.write_twin(str(tmp_path), 21, 16 << 20, dialect)
    got = Gff3AnnotationLoader(gff3).get_data()
    pd.testing.assert_frame_equal(got, GeneAnnotationLoader(gtf).get_data())
    pd.testing.assert_frame_equal(got, table_of(g3.outcome(g3.restate, open(gff3, 'rb').read())))
    pd.testing.assert_frame_equal(GeneAnnotationProcessor(gff3, verbose=False).run(), GeneAnnotationProcessor(gtf, verbose=False).run())
    named, by_id = got.gene.str.startswith('GENE'), got.gene.str.startswith('ENSG')      # the genes without a name fell back to gene_id
    assert len(got) > 5000 and (named | by_id).all() and by_id.sum() > named.sum() // 10


@pytest.fixture(scope='module')
def pipeline_files(tmp_path_factory):
    import _bam_fixtures as bf
    d = tmp_path_factory.mktemp('gff3_pipeline')
    paths = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(d / (s + '.bam'))
        bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1))
        paths.append(p)
    gff3 = str(d / 'pipeline.gff3')
    g3.write_pipeline_gff3(gff3)
    return paths, [p + '.bai' for p in paths], gff3


def test_pipeline_with_a_gff3_annotation_equals_golden(pipeline_files, tmp_path):
    from test_annotation_host import RUN_COLS, assert_same_table, golden_frame
    from test_gpu_pipeline import ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd.pipeline import prepare_inputs, run_pipeline
    bam_files, bai_files, gff3 = pipeline_files
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    all_cov, _, all_counts, _ = golden_inputs(z, [])

    out = str(tmp_path / 'prep')
    os.makedirs(out)
    cov, counts_df, genes_df, exon_df, sample_ids = prepare_inputs(bam_files, bai_files, gff3, out, minimax_coverage=minimax, verbose=False)
    assert sample_ids == samples
    assert_same_cov(cov, cov_e)
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))

    out = str(tmp_path / 'out')
    os.makedirs(out)
    model, estimates, cov, counts_df, genes_df, exon_df, sample_ids = run_pipeline(
        bam_files, bai_files, gff3, out, degnorm_iter=ITER, nmf_iter=NMF_ITER, minimax_coverage=minimax, verbose=False)
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_cov(cov, cov_e)
    ref = GeneNMFOA(degnorm_iter=ITER, nmf_iter=NMF_ITER)
    ref.run(cov_e, reads_dat=counts_e[samples].values.astype(np.float64))
    np.testing.assert_array_equal(model.rho, ref.rho)
    np.testing.assert_array_equal(model.x_adj, ref.x_adj)

    # the command line with -g x.gff3 writes the same files
    out_cli = str(tmp_path / 'cli_out')
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd', '--bam-files'] + bam_files + ['--bai-files'] + bai_files +
                       ['-g', gff3, '-o', out_cli, '--iter', str(ITER), '--nmf-iter', str(NMF_ITER), '--minimax-coverage', str(minimax)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    for name in RESULT_FILES + ['gene_exon_metadata.csv', 'read_counts.csv']:
        with open(os.path.join(out, name), 'rb') as fa, open(os.path.join(out_cli, name), 'rb') as fb:
            assert fa.read() == fb.read(), name
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out_cli, 'gene_exon_metadata.csv')), golden_frame(z, 'exon', RUN_COLS).reset_index(drop=True))
    pd.testing.assert_frame_equal(pd.read_csv(os.path.join(out_cli, 'read_counts.csv')), all_counts)
    for c in z['chroms'].tolist():
        with open(os.path.join(out_cli, c, 'coverage_matrices_{0}.pkl'.format(c)), 'rb') as f:
            assert_same_cov(pickle.load(f), OrderedDict((g, all_cov[g]) for g in z['pkl_{0}_genes'.format(c)].tolist()))
    di = pd.read_csv(os.path.join(out_cli, RESULT_FILES[0]))
    assert di.gene.tolist() == list(cov_e)
    np.testing.assert_allclose(di[samples].values, ref.rho, rtol=1e-12, atol=0)              # the CSV's decimal round trip
