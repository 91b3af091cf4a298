"""
The cases of the coverage-text formatter (csrc/dn_text.hip), shared by tests/test_text_host.py (the host build against
Python's '%.5f' and against pandas) and tests/test_gpu_text.py (the device against the host build).

POOL is every value the rule has to get right, the special ones first: carries into and across the integer part, signed
zeros, a subnormal, the integers around 2^53, the largest doubles below 2^63; every multiple of 1/64 in [0, 64) with both
signs (the odd ones are exact ties at the fifth decimal); every odd multiple of 5e-6 below 1 (decimal ties that no double
holds exactly); integer counts; 200 000 seeded values over magnitudes 1e-7 to 1e11.

CASES[name] = (p, matrices, indices of the genes built to be flagged).  A shape case p x L is a batch of matrices of that
shape filled from POOL in order: the three large shapes walk the whole pool, the four small ones its first values.  `mixed`
has the lengths side by side, an empty gene in the middle, more lines than five measure blocks; `flagged` has a NaN, both
infinities and 2^63 in four of its nine genes.
"""
import functools
import io
import math

import numpy as np
import pandas as pd

SHAPES = [(2, 1), (2, 63), (3, 64), (3, 65), (10, 257), (64, 130), (256, 70)]
SPECIAL = [0.999995, 0.9999949999, 9.999999, 99999.999995, -0.0, -1e-9, 5e-324, 2.0 ** 53 - 1, 2.0 ** 53 + 1, 1e15 + 0.5, 2.0 ** 62,
           math.nextafter(2.0 ** 63, 0.0), -math.nextafter(2.0 ** 63, 0.0), 0.0, 1.0, 999999999.0, 1e9, 999999999999999999.0, 1e18,
           2.2250738585072014e-308, 0.5e-5, 1.5e-5, 2.5e-5, -0.999995, -99999.999995]
MIXED_LENGTHS = [1, 63, 700, 64, 0, 65, 257, 130, 70]
FLAGGED = {1: float('nan'), 3: float('inf'), 4: float('-inf'), 8: 2.0 ** 63}


def _pool():
    rng = np.random.default_rng(20)
    sixty_fourths = np.arange(4096) / 64.0
    ties = np.arange(1, 200000, 2) * 5e-6
    counts = rng.integers(0, 5000, 5000).astype(np.float64)
    seeded = rng.choice([-1.0, 1.0], 200000) * 10.0 ** rng.uniform(-7, 11, 200000) * rng.uniform(0.5, 1.5, 200000)
    return np.concatenate([SPECIAL, sixty_fourths, -sixty_fourths, ties, counts, seeded])


POOL = _pool()


def _take(first, p, L):
    idx = (first + np.arange(p * L)) % POOL.size
    return POOL[idx].reshape(p, L)


def _cases():
    cases = {}
    for p, L in SHAPES:
        n = max(64 if p * L < 200 else 3, -(-POOL.size // (p * L)) if p * L >= 2000 else 0)
        cases['{0}x{1}'.format(p, L)] = (p, [_take(k * p * L, p, L) for k in range(n)], set())
    first, mats = 0, []
    for L in MIXED_LENGTHS:
        mats.append(_take(first, 3, L))
        first += 3 * L
    cases['mixed'] = (3, mats, set())
    mats = [_take(1000 + 200 * k, 4, 40 + k).copy() for k in range(9)]
    mats[1][1, 7] = FLAGGED[1]
    mats[3][0, 0] = FLAGGED[3]
    mats[4][3, -1] = FLAGGED[4]
    mats[8][2, 10] = FLAGGED[8]
    cases['flagged'] = (4, mats, set(FLAGGED))
    return cases


CASES = _cases()


def python_text(mat):
    """The body of the file of one p x L matrix by Python's own '%.5f'."""
    p, L = mat.shape
    if L == 0:
        return b''
    fmt = ' '.join(['%.5f'] * p) + '\n'
    cols = mat.T.tolist()
    return ''.join([fmt % tuple(c) for c in cols]).encode('ascii')


def pandas_text(mat):
    """The same by the reference's call, without the header line."""
    s = io.StringIO()
    pd.DataFrame(mat.T).to_csv(s, index=None, header=False, sep=' ', float_format='%.5f')
    return s.getvalue().encode('ascii')


@functools.lru_cache(maxsize=None)
def expected(name):
    """(pieces, offsets, flags) of a case: computed once, read by every test that needs it."""
    p, mats, flagged = CASES[name]
    pieces = [b'' if k in flagged else python_text(m) for k, m in enumerate(mats)]
    off = np.concatenate([[0], np.cumsum([len(b) for b in pieces])]).astype(np.int64)
    flags = np.array([1 if k in flagged else 0 for k in range(len(mats))], dtype=np.uint8)
    return pieces, off, flags
