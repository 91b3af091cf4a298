"""
k_row_max (csrc/dn_outer.hip) against numpy, through the test seam (dn_debug_peek): the kernel runs once per upload, for every
cohort width (finish_upload launches it whatever p is, wide cohorts included), and writes the row maxima behind the
0.1 * max(F) threshold and the per-gene flag that lets the NMF pass read the counts as 16-bit integers.  Neither comes back
through any other entry point.

A row is read in five segments -- a scalar head up to the next 16-byte boundary, loops of eight, four and one 16-byte loads
per lane, a scalar tail -- and a wave goes on to row w + 4, a workgroup to gene b + gridDim.  Every gene here is background
(whole numbers in [0, 1000]) plus ONE needle, and every needle changes the gene's maximum or its flag, so an element that
some segment skips or reads twice with the wrong index shows in the gene that has its needle there.  Needle columns: the first
and the last eight, both sides of every multiple of 256 floats near either end of the row (the loops hand over at multiples
of 64 16-byte loads past the head; the head is 0 to 3 floats, so columns 256 m - 1 .. 256 m + 3 hold both sides of the
hand-over for every alignment, and the head's own boundary lies in the first eight), and 64 random ones.  Every column is
taken in every row class (rows 0 to 3, a row of a wave's second trip, the last row).  Lengths straddle 64, 192, 256, 448 and 512 16-byte loads per row for every alignment; odd lengths give the
rows of one gene all four alignments.

Reference: numpy's float32 row maximum and all(0 <= v <= 65535 and v == trunc(v)), compared exactly.
"""
import numpy as np
import pytest

from degnorm_amd import _lib

pytestmark = pytest.mark.gpu


def _span(a, b):
    return list(range(a, b + 1))


LENGTHS = [1, 2, 3, 4, 5, 7, 8] + _span(255, 261) + _span(767, 773) + _span(1023, 1029) + _span(1791, 1797) + _span(2047, 2053) + [4099, 6151]
COHORTS = (2, 3, 5, 7, 64, 65)
# what a needle does: 60000 and 65535 raise the maximum and keep the flag; 65536 and 1000.5 raise it and clear the flag; 0.5 and
# -1 (an upload takes any float32) leave the maximum alone and clear the flag
NEEDLES = np.array([60000.0, 65535.0, 65536.0, 1000.5, 0.5, -1.0], np.float32)
N_BACKGROUNDS = 7


def needle_columns(L, rng):
    """(structured, random) needle columns of a row of L floats."""
    cols = set(range(min(8, L))) | set(range(max(0, L - 8), L))
    chunks = (L + 255) // 256
    for m in [1] + list(range(max(1, chunks - 10), chunks + 1)):
        cols |= {c for c in range(256 * m - 1, 256 * m + 4) if 0 <= c < L}
    extra = rng.choice(L, min(L, 64), replace=False)
    return sorted(cols), sorted(set(int(c) for c in extra) - cols)


def row_classes(p):
    return sorted(set(range(min(4, p))) | ({min(p - 1, 5)} if p > 4 else set()) | {p - 1})


def cohort(L, p, seed):
    """(coverage n x p x L float32, needle table): one gene per (needle column, row class), the needle values in turn."""
    rng = np.random.default_rng(seed)
    structured, extra = needle_columns(L, rng)
    rows = row_classes(p)
    where = [(c, r, (ci + ri) % len(NEEDLES)) for ci, c in enumerate(structured + extra) for ri, r in enumerate(rows)]
    n = len(where)
    back = rng.integers(0, 1001, (N_BACKGROUNDS, p, L)).astype(np.float32)
    cov = back[np.arange(n) % N_BACKGROUNDS]
    g = np.arange(n)
    cov[g, [w[1] for w in where], [w[0] for w in where]] = NEEDLES[[w[2] for w in where]]
    return cov, where


def reference(cov):
    whole = np.equal(cov, np.trunc(cov)).all(axis=(1, 2))
    return cov.max(axis=2), (whole & (cov.min(axis=(1, 2)) >= 0) & (cov.max(axis=(1, 2)) <= 65535)).astype(np.int32)


def check(dev, cov, what):
    n, p, L = cov.shape
    dev.upload_packed(cov.reshape(-1), np.full(n, L, np.int64), p)
    want_max, want_x16 = reference(cov)
    got_max, got_x16 = dev.debug_peek('rowmax'), dev.debug_peek('x16')
    bad = np.argwhere(got_max != want_max)
    assert bad.size == 0, '{0}: {1} row maxima differ, first at gene {2} row {3}: device {4}, numpy {5}'.format(
        what, len(bad), bad[0][0], bad[0][1], got_max[tuple(bad[0])], want_max[tuple(bad[0])])
    bad = np.flatnonzero(got_x16 != want_x16)
    assert bad.size == 0, '{0}: {1} 16-bit flags differ, first at gene {2}: device {3}, numpy {4}'.format(
        what, len(bad), bad[0], got_x16[bad[0]], want_x16[bad[0]])
    return want_max, want_x16


@pytest.fixture(scope='module')
def dev():
    d = _lib.Device(0)
    yield d
    d.close()


def test_the_needles_cover_what_they_claim():
    """Every needle changes its gene's maximum or flag; each value and each row class occurs at every length that has room."""
    for L, ps in ((1, (2, 64)), (5, (3, 7)), (259, (5, 64)), (2049, (7,)), (6151, (2, 7))):
        for p in ps:
            cov, where = cohort(L, p, 1)
            plain = cov.copy()
            g = np.arange(len(where))
            rows, cols = [w[1] for w in where], [w[0] for w in where]
            plain[g, rows, cols] = 7.0
            (m0, f0), (m1, f1) = reference(plain), reference(cov)
            assert np.all((m0[g, rows] != m1[g, rows]) | (f0 != f1)) and np.all(f0 == 1)
            assert {w[1] for w in where} == set(row_classes(p))
            if L >= 5:
                assert {w[2] for w in where} == set(range(len(NEEDLES))) and set(f1) == {0, 1}
            covered = {w[0] for w in where}
            assert covered >= set(range(min(8, L))) | set(range(max(0, L - 8), L))
            for head in range(4):                                      # both sides of every hand-over of a row with this head
                n4 = (L - head) // 4
                for k in sorted({512 * (n4 // 512), 512 * ((n4 - 1) // 512), 256 * (n4 // 256), 256 * ((n4 - 1) // 256), 64 * (n4 // 64)}):
                    for c in (head + 4 * k - 1, head + 4 * k):
                        assert not (0 <= c < L) or c in covered, (L, p, head, k, c)


@pytest.mark.parametrize('p', COHORTS)
@pytest.mark.parametrize('L', LENGTHS)
def test_row_maxima_and_flags(dev, L, p):
    cov, where = cohort(L, p, 100 * L + p)
    check(dev, cov, 'L={0} p={1}'.format(L, p))


def test_more_genes_than_workgroups(dev):
    """The grid is min(n, 8 x CUs) workgroups: with more genes a workgroup goes on to gene b + gridDim, and the flags of its
    four waves (ok_w) are used again.  Tiny genes, the flag alternating from gene to gene."""
    n, p, L = 8 * 512 + 37, 5, 9
    rng = np.random.default_rng(3)
    cov = rng.integers(0, 1001, (n, p, L)).astype(np.float32)
    odd = np.arange(1, n, 2)
    cov[odd, rng.integers(0, p, odd.size), rng.integers(0, L, odd.size)] = rng.choice(NEEDLES[2:], odd.size)
    big = np.arange(0, n, 2)
    cov[big, rng.integers(0, p, big.size), rng.integers(0, L, big.size)] = rng.choice(NEEDLES[:2], big.size)
    _, x16 = check(dev, cov, 'grid-stride')
    assert np.array_equal(x16, (np.arange(n) % 2 == 0).astype(np.int32))
