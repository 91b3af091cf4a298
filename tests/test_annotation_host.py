"""
Host side of the annotation stage (degnorm_amd.loaders, degnorm_amd.gene_processing), no device: the loader's argument
checks, the table work of GeneAnnotationProcessor after the load against the reference's goldens
(tests/golden/annotation.npz, made by tests/golden/make_golden_pipeline.py), the window cutter, the interning of names,
and the rule that there is no CPU fallback for the scan itself.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from conftest import golden, GOLDEN                                    # noqa: E402
from degnorm_amd import _lib, loaders                                  # noqa: E402
from degnorm_amd.gene_processing import GeneAnnotationProcessor        # noqa: E402
from degnorm_amd.loaders import GeneAnnotationLoader                   # noqa: E402
from degnorm_amd.utils import subset_to_chrom                          # noqa: E402

DATA_COLS = ['chr', 'start', 'end', 'gene']
RUN_COLS = ['chr', 'start', 'end', 'gene', 'gene_start', 'gene_end']
FIXTURES = ['chr1_small', 'hard', 'pipeline']


def golden_frame(z, key, cols):
    """A table of annotation.npz / pipeline.npz as the DataFrame the reference returned: str columns as object, its index."""
    df = pd.DataFrame({c: z['{0}_{1}'.format(key, c)].astype(object) if z['{0}_{1}'.format(key, c)].dtype.kind == 'U'
                       else z['{0}_{1}'.format(key, c)] for c in cols})
    df.index = z[key + '_index']
    return df


def assert_same_table(df, expect):
    """Equal values, column order and dtypes; where the reference's index is 0 .. n-1 ours must be a RangeIndex."""
    pd.testing.assert_frame_equal(df, expect)
    assert [str(t) for t in df.dtypes] == [str(t) for t in expect.dtypes]
    if np.array_equal(expect.index, np.arange(len(expect))):
        assert isinstance(df.index, pd.RangeIndex)


def test_loader_argument_errors(tmp_path):
    with pytest.raises(ValueError, match='data type not understood'):
        GeneAnnotationLoader(17)
    with pytest.raises(FileNotFoundError, match='not found'):
        GeneAnnotationLoader(str(tmp_path / 'missing.gtf'))
    other = tmp_path / 'genes.gff3'
    other.write_text('x\n')
    with pytest.raises(ValueError, match='does not end with .gtf'):
        GeneAnnotationLoader(str(other))
    ok = GeneAnnotationLoader(os.path.join(GOLDEN, 'chr1_small.gtf'))
    assert ok.filename.endswith('chr1_small.gtf') and ok.window_bytes == loaders.WINDOW_BYTES


@pytest.mark.parametrize('name', FIXTURES)
def test_processing_after_load_equals_reference(name):
    z = golden('annotation')
    data = golden_frame(z, name + '_data', DATA_COLS)
    expect = golden_frame(z, name + '_run', RUN_COLS)
    gap = GeneAnnotationProcessor(os.path.join(GOLDEN, name + '.gtf'), verbose=False)
    assert_same_table(gap.process(gap._subset(data)), expect)
    # the two static steps on their own
    kept = GeneAnnotationProcessor.remove_multichrom_genes(data)
    per_gene = data.groupby('gene').chr.nunique()
    assert set(kept.gene) == set(per_gene[per_gene == 1].index) and kept.index.isin(data.index).all()
    outline = GeneAnnotationProcessor.gene_outline(kept)
    want = expect[['chr', 'gene', 'gene_start', 'gene_end']].drop_duplicates().sort_values(['chr', 'gene']).reset_index(drop=True)
    assert_same_table(outline, want)


def test_chromosome_subset_comes_before_multichrom_removal():
    z = golden('annotation')
    data = golden_frame(z, 'hard_data', DATA_COLS)
    expect = golden_frame(z, 'hard_sub_run', RUN_COLS)
    gap = GeneAnnotationProcessor(os.path.join(GOLDEN, 'hard.gtf'), chroms=['1', 'X'], verbose=False)
    got = gap.process(gap._subset(data))
    assert_same_table(got, expect)
    assert 'TWO' in set(got.gene) and 'TWO' not in set(z['hard_run_gene'].tolist())
    assert GeneAnnotationProcessor('x.gtf', chroms='1').chroms == ['1']


def test_empty_results_raise_the_reference_errors():
    z = golden('annotation')
    data = golden_frame(z, 'chr1_small_data', DATA_COLS)
    with pytest.raises(ValueError, match='Chromosome subsetting resulted in an empty DataFrame!'):
        GeneAnnotationProcessor('x.gtf', chroms=['nope'], verbose=False)._subset(data)
    with pytest.raises(ValueError, match='Exon DataFrame is empty!'):
        GeneAnnotationProcessor('x.gtf', verbose=False)._subset(data.iloc[:0])
    sub = subset_to_chrom(data, 'chr1', reindex=True)
    assert isinstance(sub.index, pd.RangeIndex) and len(sub) == len(data)


def test_gene_outline_makes_no_python_call_per_gene(monkeypatch):
    n = 20000
    df = pd.DataFrame({'chr': 'c', 'start': np.arange(n) * 10 + 1, 'end': np.arange(n) * 10 + 5, 'gene': ['g{0}'.format(k // 2) for k in range(n)]})
    calls = []
    monkeypatch.setattr(pd.core.groupby.DataFrameGroupBy, 'apply', lambda *a, **k: calls.append(1))
    out = GeneAnnotationProcessor.gene_outline(df)
    assert not calls and len(out) == n // 2
    assert out.gene_start.dtype == np.int64 and out.gene_end.dtype == np.int64
    k = out.gene.tolist().index('g7')
    assert (out.gene_start[k], out.gene_end[k]) == (141, 155)


def test_windows_end_at_line_ends(tmp_path):
    lines = [b'a' * k for k in (3, 0, 50, 7, 1200, 2, 9)]
    for tail in (b'\n', b''):
        p = tmp_path / 'w.txt'
        p.write_bytes(b'\n'.join(lines) + tail)
        for window in (1, 5, 64, 1000, 1 << 20):
            wins = list(loaders.iter_windows(str(p), window))
            assert b''.join(wins) == p.read_bytes()
            assert all(w.endswith(b'\n') for w in wins[:-1]) and all(len(w) > 0 for w in wins)


def test_names_that_share_a_hash_stay_apart():
    text = b'alpha beta alpha gamma beta alpha'
    a = np.frombuffer(text, dtype=np.uint8)
    words = text.split(b' ')
    beg = np.cumsum([0] + [len(w) + 1 for w in words[:-1]]).astype(np.int64)
    length = np.array([len(w) for w in words], dtype=np.int64)
    honest = np.array([hash(w) & 0xffffffffffffffff for w in words], dtype=np.uint64)
    for hashes in (honest, np.zeros(len(words), dtype=np.uint64), np.array([1, 2, 1, 1, 2, 1], dtype=np.uint64)):      # honest, all lengths mixed, alpha / gamma mixed
        table = {b'seen': 0}
        codes = loaders.intern_spans(a, beg, length, hashes, table)
        assert list(table) == [b'seen', b'alpha', b'beta', b'gamma']
        assert codes.tolist() == [1, 2, 1, 3, 2, 1]


def test_scan_has_no_cpu_fallback():
    if _lib.device_count() > 0:
        pytest.skip('a GPU is visible here')
    with pytest.raises(_lib.DegnormAmdError):
        GeneAnnotationLoader(os.path.join(GOLDEN, 'chr1_small.gtf')).get_data()
    with pytest.raises(_lib.DegnormAmdError):
        GeneAnnotationProcessor(os.path.join(GOLDEN, 'chr1_small.gtf'), verbose=False).run()
