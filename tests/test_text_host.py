"""
Host build of the coverage-text formatter (dn_cov_text_host, csrc/dn_text.hip and dn_text.hpp; degnorm_amd.data_access.cov_text
with host=True), no device: every case of tests/_text_cases.py against Python's own '%.5f', byte for byte, with offsets and
flags; whole matrices against the pandas call the reference writes its files with; the batch cut into three; and every early
refusal of both entries with its status and message.
"""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _text_cases as tc                                       # noqa: E402
from degnorm_amd import _lib, data_access as da                # noqa: E402


def host_result(name):
    p, mats, _ = tc.CASES[name]
    with da.cov_text(mats, host=True) as t:
        return [bytes(t.piece(k)) for k in range(len(mats))], t.off.copy(), t.flag.copy(), bytes(t.view)


def test_the_cases_are_what_they_claim():
    assert [(p, m[0].shape[1]) for p, m, _ in (tc.CASES['{0}x{1}'.format(*s)] for s in tc.SHAPES)] == tc.SHAPES
    for s in [(10, 257), (64, 130), (256, 70)]:                 # the large shapes walk the whole pool
        p, mats, _ = tc.CASES['{0}x{1}'.format(*s)]
        assert sum(m.size for m in mats) >= tc.POOL.size
    pool = set(tc.POOL.tolist())
    assert all(v in pool for v in tc.SPECIAL) and 2.0 ** 62 in pool and 63.984375 in pool and -63.984375 in pool
    # an odd multiple of 1/64 is an exact tie at the fifth decimal; an odd multiple of 5e-6 never is, as a double
    assert Fraction(3 / 64.0) * 10 ** 5 % 1 == Fraction(1, 2)
    assert Fraction(15e-6) * 10 ** 5 % 1 != Fraction(1, 2) and 15e-6 in pool
    assert np.isfinite(tc.POOL).all() and np.abs(tc.POOL).max() < 2.0 ** 63 and np.abs(tc.POOL).max() >= 2.0 ** 63 - 1024
    p, mats, flagged = tc.CASES['mixed']
    lens = [m.shape[1] for m in mats]
    assert 0 in lens[1:-1] and sum(lens) > 5 * 256 and flagged == set()
    p, mats, flagged = tc.CASES['flagged']
    bad = {k for k, m in enumerate(mats) if not (np.isfinite(m).all() and (np.abs(m) < 2.0 ** 63).all())}
    assert bad == flagged == {1, 3, 4, 8}
    for name, (p, mats, flagged) in tc.CASES.items():
        if name != 'flagged':
            assert flagged == set() and all(np.isfinite(m).all() for m in mats)
    # the restatement itself: ties go to even, the sign of a negative zero stays
    assert tc.python_text(np.array([[1 / 64.0], [3 / 64.0], [-0.0], [-1e-9], [0.999995], [99999.999995], [5e-324]])) \
        == b'0.01562 0.04688 -0.00000 -0.00000 0.99999 100000.00000 0.00000\n'


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_host_text_equals_python(name):
    pieces, off, flag, whole = host_result(name)
    e_pieces, e_off, e_flag = tc.expected(name)
    assert set(np.flatnonzero(flag).tolist()) == tc.CASES[name][2]             # nothing passes by flagging
    assert flag.tolist() == e_flag.tolist() and off.tolist() == e_off.tolist()
    for k, (got, want) in enumerate(zip(pieces, e_pieces)):
        assert got == want, (name, k)
    assert whole == b''.join(e_pieces)


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_host_text_equals_pandas_on_whole_matrices(name):
    p, mats, flagged = tc.CASES[name]
    pieces = host_result(name)[0]
    which = range(len(mats)) if name in ('10x257', 'mixed', 'flagged') else [0, len(mats) - 1]
    for k in which:
        if k not in flagged and mats[k].shape[1] > 0:
            assert pieces[k] == tc.pandas_text(mats[k]), (name, k)


def test_three_batches_equal_one():
    p, mats, _ = tc.CASES['mixed']
    budget = 8 * sum(m.size for m in mats) // 3
    one, one_flag, n_one = da.cov_text_pieces(mats, host=True)
    three, three_flag, n_three = da.cov_text_pieces(mats, host=True, batch_bytes=budget)
    assert (n_one, n_three) == (1, 3)
    assert three == one == tc.expected('mixed')[0] and three_flag.tolist() == one_flag.tolist()


def test_other_number_types_and_strides():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 300, (4, 50))
    mats = [base.astype(np.int64), base.astype(np.float32), np.asfortranarray(base.astype(np.float64)), base.astype(np.float64)[:, ::2]]
    with da.cov_text(mats, host=True) as t:
        for k, m in enumerate(mats):
            assert bytes(t.piece(k)) == tc.python_text(np.asarray(m, dtype=np.float64))
    with pytest.raises(ValueError, match='disagree on the number of samples'):
        da.cov_text([np.zeros((2, 3)), np.zeros((3, 3))], host=True)
    with pytest.raises(ValueError, match='2-d'):
        da.cov_text([np.zeros(3)], host=True)
    with pytest.raises(ValueError, match='no matrices'):
        da.cov_text([], host=True)


# -- refusals: status and message, before any work ----------------------------------------------------------------------

def _call(fn_name, x, n_x, n_genes, p, beg, lens, null=()):
    lib = _lib.load()
    x, beg, lens = np.asarray(x, np.float64), np.asarray(beg, np.int64), np.asarray(lens, np.int64)
    off, flag, h = np.zeros(n_genes + 1, np.int64), np.zeros(n_genes, np.uint8), ctypes.c_void_p()
    args = {'x': _lib._p(x, ctypes.c_double), 'beg': _lib._p(beg, ctypes.c_int64), 'len': _lib._p(lens, ctypes.c_int64),
            'off': _lib._p(off, ctypes.c_int64), 'flag': _lib._p(flag, ctypes.c_uint8), 'text': ctypes.byref(h)}
    for k in null:
        args[k] = None
    a = [args['x'], n_x, n_genes, p, args['beg'], args['len'], args['off'], args['flag'], args['text']]
    rc = lib.dn_cov_text_host(*a) if fn_name == 'dn_cov_text_host' else lib.dn_cov_text(0, *(a + [None]))
    assert not h.value
    return rc, lib.dn_last_error().decode()


X8 = np.arange(8.0)
REFUSALS = [
    ('null_x', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 2], null=('x',)), 'null argument'),
    ('null_beg', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 2], null=('beg',)), 'null argument'),
    ('null_len', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 2], null=('len',)), 'null argument'),
    ('null_off', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 2], null=('off',)), 'null argument'),
    ('null_flag', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 2], null=('flag',)), 'null argument'),
    ('null_text', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 2], null=('text',)), 'null argument'),
    ('p_1', dict(x=X8, n_x=8, n_genes=2, p=1, beg=[0, 4], lens=[2, 2]), 'fewer than 2 samples'),
    ('p_0', dict(x=X8, n_x=8, n_genes=2, p=0, beg=[0, 4], lens=[2, 2]), 'fewer than 2 samples'),
    ('p_4097', dict(x=X8, n_x=8, n_genes=2, p=4097, beg=[0, 4], lens=[0, 0]), 'more than 4096 samples'),
    ('no_values', dict(x=X8, n_x=0, n_genes=2, p=2, beg=[0, 0], lens=[0, 0]), 'bad argument'),
    ('no_genes', dict(x=X8, n_x=8, n_genes=0, p=2, beg=[0], lens=[0]), 'bad argument'),
    ('negative_length', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, -1]), 'gene 1 has a negative length'),
    ('negative_begin', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[-1, 4], lens=[2, 2]), 'gene 0 leaves the buffer'),
    ('begin_beyond', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 9], lens=[2, 0]), 'gene 1 leaves the buffer'),
    ('end_beyond', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 4], lens=[2, 3]), 'gene 1 leaves the buffer'),
    ('overlap', dict(x=X8, n_x=8, n_genes=2, p=2, beg=[0, 3], lens=[2, 2]), 'genes 0 and 1 overlap'),
    ('overlap_unordered', dict(x=X8, n_x=8, n_genes=3, p=2, beg=[4, 8, 2], lens=[2, 0, 2]), 'genes 0 and 2 overlap'),
]


@pytest.mark.parametrize('fn_name', ['dn_cov_text_host', 'dn_cov_text'])
@pytest.mark.parametrize('case', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_work(fn_name, case):
    _, kw, text = case
    rc, message = _call(fn_name, **kw)
    assert rc == _lib.DN_E_INVALID and message == '{0}: {1}'.format(fn_name, text)


def test_accepted_layouts():
    # genes in any order of their begins, gaps between them, an empty gene at the very end of the buffer
    x = np.arange(12.0)
    lib = _lib.load()
    beg, lens = np.array([6, 12, 0], np.int64), np.array([2, 0, 2], np.int64)
    off, flag, h = np.zeros(4, np.int64), np.zeros(3, np.uint8), ctypes.c_void_p()
    rc = lib.dn_cov_text_host(_lib._p(x, ctypes.c_double), 12, 3, 2, _lib._p(beg, ctypes.c_int64), _lib._p(lens, ctypes.c_int64),
                              _lib._p(off, ctypes.c_int64), _lib._p(flag, ctypes.c_uint8), ctypes.byref(h))
    assert rc == _lib.DN_OK and h.value
    text = ctypes.string_at(lib.dn_text_bytes(h), lib.dn_text_size(h))
    lib.dn_text_free(h)
    assert text == b'6.00000 8.00000\n7.00000 9.00000\n0.00000 2.00000\n1.00000 3.00000\n' and off.tolist() == [0, 32, 32, 64]
    lib.dn_text_free(None)


def test_no_device_is_an_error_not_a_fallback():
    if _lib.device_count() > 0:
        with da.cov_text([np.ones((2, 3))]) as t:
            assert bytes(t.view) == b'1.00000 1.00000\n' * 3
    else:
        with pytest.raises(_lib.DegnormAmdError, match='no HIP device'):
            da.cov_text([np.ones((2, 3))])
