"""bench.py's post-clock accounting helpers that need no GPU: the tie count of get_high_coverage_idx and the parity sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_tie_sensitive_genes_counts_columns_on_the_threshold():
    import bench
    p = 3
    a = np.array([[100., 10., 50., 9.], [5., 3., 2., 1.], [1., 1., 1., 1.]], dtype=np.float32)      # column 1: 10 x 10 == 100 -> on the threshold
    b = np.array([[100., 11., 50.], [5., 3., 2.], [1., 1., 1.]], dtype=np.float32)                  # no column at 10
    c = np.array([[40., 4., 4., 39.], [7., 1., 1., 1.], [2., 2., 2., 2.]], dtype=np.float32)        # two columns at max / 10
    packed = np.concatenate([m.ravel() for m in (a, b, c)])
    out = bench.tie_sensitive_genes(packed, [4, 3, 4], p, np.ones(p))
    assert out['genes'] == 2 and out['columns'] == 3 and out['of_genes'] == 3
    # a scale factor that is not a power of two keeps exact ties of the SAME row on the threshold (the quotient is monotone and the
    # two sides round alike), which is why such genes flip on the last bit of s
    out = bench.tie_sensitive_genes(packed, [4, 3, 4], p, np.array([1.1, 1.0, 1.0]))
    assert out['genes'] >= 1


def test_parity_sample_spans_all_lengths():
    import bench
    lengths = np.arange(200, 5000, 7)
    pick = bench.parity_sample(lengths, 160)
    assert len(pick) <= 160 and len(np.unique(pick)) == len(pick)
    assert lengths[pick].min() == lengths.min() and lengths[pick].max() == lengths.max()
    assert len(bench.parity_sample(lengths[:10], 160)) == 10


def test_algorithmic_bytes_formula():
    """bytes_g = 4 p [ 2 L_g + sum_k n_{g,k} (3 T + 3) ]."""
    import bench
    trace = np.zeros((2, 8), dtype=np.int32)
    trace[:, 2] = [1000, 0]
    lengths = np.array([500., 300.])
    assert bench.algorithmic_bytes(trace, lengths, 10, 100) == 4 * 10 * (2 * 500 + 1000 * 303) + 4 * 10 * (2 * 300)
    assert bench.algorithmic_bytes(trace, lengths, 10, 100, mask=np.array([False, True])) == 4 * 10 * 600


class _Shard(object):
    """The attributes of a ShardedNMFOA that a step leaves for its caller (after fetch_state)."""

    def __init__(self, ids, p=3, iters=2):
        ids = np.asarray(ids, dtype=np.int64)
        self.p, self.degnorm_iter, self.n_local, self.global_ids = p, iters, len(ids), ids
        self.rho = ids[:, None] + np.linspace(0.1, 0.3, p)[None, :]
        self.x_adj = 2.0 * self.rho
        self.x_weighted = 3.0 * self.rho
        self.ran_baseline_selection = (ids[:, None] + np.arange(iters)[None, :]) % 2 == 1
        self.scale_factors = np.linspace(0.9, 1.1, p)


class _Gather(object):
    """gather_objects of two ranks played in one process: rank 1 leaves its object in `box`, rank 0 gets both."""

    def __init__(self, rank, box):
        self.rank, self.box = rank, box

    def gather_objects(self, obj):
        if self.rank == 1:
            self.box.append(obj)
        return [obj] + self.box if self.rank == 0 else [None, obj]


def test_step_outputs_puts_every_rank_in_global_gene_order(tmp_path):
    import bench
    box = []
    assert bench.step_outputs(_Shard([1, 3]), _Gather(1, box), 2) is None
    out = bench.step_outputs(_Shard([4, 0, 2]), _Gather(0, box), 2)
    assert out['gene_ids'].tolist() == [0, 1, 2, 3, 4]
    np.testing.assert_array_equal(out['rho'][:, 0], np.arange(5) + 0.1)
    np.testing.assert_array_equal(out['x_adj'], 2.0 * out['rho'])
    assert out['rho'].dtype == np.float64 and out['ran_baseline_selection'].dtype == np.float32
    np.testing.assert_array_equal(out['ran_baseline_selection'][:, 0], np.arange(5) % 2)
    info = bench.dump_outputs(out, str(tmp_path / 'd'))
    assert info['sampled_genes'] is None
    names = sorted(f for f in os.listdir(str(tmp_path / 'd')))
    assert names == ['ran_baseline_selection.npy', 'rho.npy', 'scale_factors.npy', 'x_adj.npy', 'x_weighted.npy']
    for n in names:
        arr = np.load(str(tmp_path / 'd' / n))
        assert arr.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(arr, out[n[:-4]])


def test_dump_outputs_keeps_to_the_byte_cap_with_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 40000)
    out = bench.step_outputs(_Shard(np.arange(1000)), _Gather(0, []), 1)
    info = [bench.dump_outputs(out, str(tmp_path / d)) for d in ('a', 'b')]
    k = info[0]['sampled_genes']
    assert 0 < k < 1000 and info[1]['sampled_genes'] == k
    total = sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a')))
    assert total <= 40000
    ids = np.load(str(tmp_path / 'a' / 'gene_ids.npy'))
    np.testing.assert_array_equal(ids, np.load(str(tmp_path / 'b' / 'gene_ids.npy')))
    assert len(ids) == k and np.all(np.diff(ids) > 0)
    np.testing.assert_array_equal(np.load(str(tmp_path / 'a' / 'rho.npy')), out['rho'][ids.astype(np.int64)])
    assert np.load(str(tmp_path / 'a' / 'scale_factors.npy')).shape == (3,)


def test_steps_must_be_positive():
    import pytest
    import bench
    assert bench.parse(['--steps', '7']).steps == 7
    with pytest.raises(SystemExit):
        bench.parse(['--steps', '0'])


def test_full_is_off_by_default():
    import bench
    assert bench.parse(['--gpus', '1', '--steps', '3', '--warmup', '2']).full is False
    assert bench.parse(['--full']).full is True
