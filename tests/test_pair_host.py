"""
Mate pairing without a GPU: bam.pair_rows, the host build of csrc/dn_pair.hip (the chunk extraction and the head test of the
kernels, with std::stable_sort in place of the radix sort), against numpy -- order == np.argsort(keys, kind='stable') and
pair_id == the count of key changes before each position, element for element -- on the key shapes of tests/_pair_cases.py;
and the pair option of the reader and of the command line.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _pair_cases as pc                                       # noqa: E402
from degnorm_amd import bam                                    # noqa: E402


def _check(keys, name):
    order_e, pair_id_e, n_ids_e = pc.oracle(keys)
    for given in (pc.as_array(keys), list(keys)):              # an S array, and a list of bytes
        order, pair_id, n_ids = bam.pair_rows(given)
        assert order.dtype == np.int32 and pair_id.dtype == np.int32 and len(order) == len(pair_id) == len(keys), name
        assert np.array_equal(order, order_e), name
        assert np.array_equal(pair_id, pair_id_e), name
        assert n_ids == n_ids_e, name


@pytest.mark.parametrize('name,keys', pc.key_sets(), ids=[n for n, _ in pc.key_sets()])
def test_pair_rows_equals_numpy(name, keys):
    _check(keys, name)


def test_case_list_covers_the_shapes():
    sets = dict(pc.key_sets())
    assert [len(sets['n{0}'.format(n)]) for n in range(4)] == [0, 1, 2, 3]
    for w in pc.WIDTHS:
        keys = sets['width{0}'.format(w)]
        assert set(len(k) for k in keys) == {w} and 1 < len(set(keys)) < len(keys)
    assert len(set(sets['all_equal'])) == 1 and len(set(sets['all_distinct'])) == len(sets['all_distinct'])
    assert [sets['empty_x{0}'.format(t)].count(b'') for t in (1, 2, 5)] == [1, 2, 5]
    assert {b'r1', b'r10', b'r1.a'} <= set(sets['prefix'])
    assert len(set(k[:8] for k in sets['ninth_byte'])) == 1 and len(set(k[8:9] for k in sets['ninth_byte'])) > 2
    assert len(set(k[1:] for k in sets['first_byte'])) == 1 and len(set(k[:1] for k in sets['first_byte'])) > 2
    assert max(max(k) for k in sets['high_bytes'] if k) >= 0x80
    assert sets['triple'].count(b't3') == 3 and sets['triple'].count(b'o1') == 1
    # the order the contract fixes where numpy's default would be free to differ: ties in file order, prefixes first
    order, pair_id, n_ids = bam.pair_rows([b'r10', b'r1', b'r1.a', b'r1', b''])
    assert order.tolist() == [4, 1, 3, 2, 0] and pair_id.tolist() == [0, 1, 1, 2, 3] and n_ids == 4


def test_pair_rows_random_20000():
    keys = pc.random_keys(20000, 7000, seed=5, high=True)
    assert len(set(keys)) > 6000 and len(set(len(k) for k in keys)) > 30
    _check(keys, 'random')


def test_pair_option_is_checked():
    with pytest.raises(ValueError, match="pair must be 'host' or 'device', not 'bogus'"):
        bam.NativeBamReadsProcessor('x.bam', 'x.bai', pair='bogus')


def test_device_pair_flag_reaches_run_pipeline(tmp_path, monkeypatch):
    from degnorm_amd import __main__ as cli
    from degnorm_amd import pipeline
    assert cli.argparser().parse_args([]).device_pair is False
    for name in ('a.bam', 'a.bai', 'b.bam', 'b.bai', 'g.gtf'):
        (tmp_path / name).write_bytes(b'')
    seen = []
    monkeypatch.setattr(pipeline, 'run_pipeline', lambda *a, **kw: seen.append(kw))
    base = ['--bam-files', str(tmp_path / 'a.bam'), str(tmp_path / 'b.bam'), '-g', str(tmp_path / 'g.gtf')]
    assert cli.main(base + ['-o', str(tmp_path / 'o1'), '--device-pair']) == 0
    assert cli.main(base + ['-o', str(tmp_path / 'o2'), '--device-pair', '--device-inflate', '--device-frame']) == 0
    assert cli.main(base + ['-o', str(tmp_path / 'o3')]) == 0
    assert [(kw['inflate'], kw['frame'], kw['pair']) for kw in seen] == [('host', 'host', 'device'), ('device', 'device', 'device'),
                                                                         ('host', 'host', 'host')]
