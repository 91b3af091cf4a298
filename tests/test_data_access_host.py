"""
degnorm_amd.data_access without a GPU (formatter='pandas'): the loader and the file layout.  The seeded directory of
tests/_data_access_fixtures.write_reference_dir -- what the reference's own test builds -- must give the files the real
reference wrote (tests/golden/data_access.npz, from tests/golden/make_golden_data_access.py); a second directory has
lower-case gene names, a second chromosome, a gene missing from one pickle and a sample id with a space in it; and the
three errors of the loader.  tests/test_gpu_text.py holds the device formatter to the same golden.
"""
import io
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _data_access_fixtures as daf                             # noqa: E402
from conftest import golden                                    # noqa: E402
from degnorm_amd import data_access as da                      # noqa: E402


def golden_files():
    z = golden('data_access')
    return {p: z['file_{0}'.format(k)].tobytes() for k, p in enumerate(z['paths'].tolist())}, z


@pytest.fixture(scope='module')
def reference_dir(tmp_path_factory):
    return daf.write_reference_dir(str(tmp_path_factory.mktemp('reference') / 'out'))


@pytest.fixture(scope='module')
def hard_dir(tmp_path_factory):
    return daf.write_hard_dir(str(tmp_path_factory.mktemp('hard') / 'out'))


def test_golden_exercises_rounding():
    files, z = golden_files()
    assert sorted(files) == ['chr1/GENE_1_estimated_coverage.txt', 'chr1/GENE_1_raw_coverage.txt', 'chr1/GENE_2_estimated_coverage.txt',
                             'chr1/GENE_2_raw_coverage.txt']
    est = pd.read_csv(io.BytesIO(files['chr1/GENE_2_estimated_coverage.txt']), sep=' ')
    raw = pd.read_csv(io.BytesIO(files['chr1/GENE_2_raw_coverage.txt']), sep=' ')
    assert est.shape == raw.shape == (2495, 2) and list(est.columns) == daf.REFERENCE_SAMPLES
    assert (raw.values % 1 == 0).all() and (est.values % 1 != 0).mean() > 0.99
    assert files['chr1/GENE_1_raw_coverage.txt'].startswith(b'sample_1 sample_2\n')


def test_pandas_formatter_writes_the_reference_files(reference_dir, tmp_path):
    files, z = golden_files()
    save = str(tmp_path / 'saved')
    stats = {}
    out = da.get_coverage_data(daf.REFERENCE_GENES, reference_dir, save_dir=save, formatter='pandas', stats=stats)
    assert daf.tree(save) == files
    assert list(out) == z['genes'].tolist() == daf.REFERENCE_GENES
    for g in out:
        assert sorted(out[g]) == ['estimate', 'raw']
        for kind in ('raw', 'estimate'):
            df = out[g][kind]
            assert isinstance(df, pd.DataFrame) and list(df.columns) == z['columns'].tolist() and df.shape == tuple(z['shape_' + g])
            assert df.values.dtype == np.float64
    assert stats['values'] == 2 * 2 * (225 + 2495) and stats['batches'] == 0


def test_frames_are_the_transposed_matrices(reference_dir):
    ldr = da.CoverageLoader(reference_dir).load('all')
    out = da.get_coverage_data('ALL', reference_dir)
    assert list(out) == list(ldr.cov_dict) == daf.REFERENCE_GENES
    for g in out:
        np.testing.assert_array_equal(out[g]['raw'].values, ldr.cov_dict[g]['raw'].T)
        np.testing.assert_array_equal(out[g]['estimate'].values, ldr.cov_dict[g]['estimate'].T)
    assert ldr.sample_ids == daf.REFERENCE_SAMPLES and ldr.chroms == ['chr1'] and ldr.genes == daf.REFERENCE_GENES
    assert ldr.data_dir == reference_dir and set(ldr.exon_df.gene) == set(daf.REFERENCE_GENES)


def test_one_gene_in_any_letter_case(reference_dir, tmp_path):
    files, _ = golden_files()
    save = str(tmp_path / 'deep' / 'er' / 'saved')                  # directories are created as needed
    out = da.get_coverage_data('gene_1', reference_dir, save_dir=save, formatter='pandas')
    assert list(out) == ['GENE_1']
    assert daf.tree(save) == {p: b for p, b in files.items() if 'GENE_1' in p}


def test_hard_directory(hard_dir, tmp_path):
    ldr = da.CoverageLoader(hard_dir).load('all')
    assert ldr.sample_ids == daf.HARD_SAMPLES and ldr.chroms == ['chr1', 'chr2']
    assert ldr.genes == ['ABC1', 'DEF2', 'GHI3', 'ONLY_RAW', 'JKL4']
    assert list(ldr.cov_dict) == ['ABC1', 'DEF2', 'GHI3', 'JKL4']      # a gene enters only when both pickles have it
    assert set(ldr.exon_df.gene) == set(ldr.genes)
    save = str(tmp_path / 'saved')
    out = da.get_coverage_data(['jkl4', 'Abc1', 'only_raw'], hard_dir, save_dir=save, formatter='pandas')
    assert list(out) == ['ABC1', 'JKL4']
    got = daf.tree(save)
    assert sorted(got) == ['chr1/ABC1_estimated_coverage.txt', 'chr1/ABC1_raw_coverage.txt', 'chr2/JKL4_estimated_coverage.txt',
                           'chr2/JKL4_raw_coverage.txt']
    for path, data in got.items():
        assert data.startswith(b'"s 1" s2 s3\n')                    # pandas quotes the id that holds the separator
        back = pd.read_csv(io.BytesIO(data), sep=' ')
        assert list(back.columns) == daf.HARD_SAMPLES
        gene, kind = os.path.basename(path).split('_')[0], 'raw' if '_raw_' in path else 'estimate'
        np.testing.assert_allclose(back.values, out[gene][kind].values, rtol=0, atol=5.0000001e-6)
    assert da.header_line(daf.HARD_SAMPLES) == b'"s 1" s2 s3\n' and da.header_line(['a', 'b']) == b'a b\n'


def test_the_three_errors(reference_dir, tmp_path):
    with pytest.raises(NotADirectoryError, match='is not a directory, cannot find DegNorm output'):
        da.CoverageLoader(str(tmp_path / 'nothing_here'))
    with pytest.raises(NotADirectoryError):
        da.get_coverage_data('GENE_1', os.path.join(reference_dir, 'read_counts.csv'))
    for missing in da.REQUIRED_FILES:
        d = daf.write_reference_dir(str(tmp_path / ('without_' + missing)))
        os.remove(os.path.join(d, missing))
        with pytest.raises(ValueError, match='Missing requested files. Check that .* is a  DegNorm output directory.'):
            da.CoverageLoader(d)
    with pytest.raises(ValueError, match='Genes NOPE were not found in DegNorm output'):
        da.get_coverage_data(['GENE_1', 'nope'], reference_dir)
    with pytest.raises(ValueError, match='formatter'):
        da.get_coverage_data('GENE_1', reference_dir, formatter='numpy')


def test_command_line_with_the_pandas_formatter(reference_dir, tmp_path, capsys):
    files, _ = golden_files()
    save = str(tmp_path / 'saved')
    assert da.main(['-d', reference_dir, '-g', 'all', '-o', save, '--formatter', 'pandas']) == 0
    assert daf.tree(save) == files
    assert '2 genes' in capsys.readouterr().out
    args = da.argparser().parse_args(['-d', 'x', '-g', 'A', 'B', '-o', 'y', '--device', '1'])
    assert (args.genes, args.device, args.formatter) == (['A', 'B'], 1, 'device')
