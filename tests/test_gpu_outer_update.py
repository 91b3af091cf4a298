"""
The O(n p) kernels around the NMF pass (csrc/dn_outer.hip: k_scale_reads and k_outer_partials, k_outer_reduce, k_outer_apply,
k_init_partials <WR>, instantiated with one sample per lane for at most 64 samples and with four for 65 to 256) against
tests/_outer_restatement.py, on state planted through the test seam (dn_debug_plant): DI rows that no data set produces -- above 0.9, negative, -0.0, a single denormal, a single
non-zero entry in the last sample or in one per-lane slot --, every status and flag value, gene counts on both sides of
every block-count edge (a multiple of 4 genes, of 8 blocks, the 512-block cap) and sample counts on both sides of every
lane-slot edge.  The genes themselves are trivial (one base, constant counts): nothing here runs the NMF pass.

What is asserted, and where the numbers come from:
  * elementwise outputs (clipped rho, rho after apply, x_adj, x_weighted, ran, x_weighted of dn_outer_begin_scaled) are numpy's
    bit for bit: each is one or two correctly rounded IEEE double operations, and nothing in them can be contracted;
  * the four counts are the reference's exactly;
  * each per-sample sum S of non-negative terms satisfies |S - fsum| <= n 2^-53 fsum, the bound of ANY order of additions;
  * S equals the restatement of the device's documented summation order bit for bit, and a second call gives the same bits.
"""
import numpy as np
import pytest

import _outer_restatement as R
from degnorm_amd import _lib

pytestmark = pytest.mark.gpu

NARROW_P = (2, 3, 63, 64)
WIDE_P = (65, 127, 128, 129, 192, 193, 256)
N_LIST = (1, 3, 4, 5, 32, 33, 60, 2047, 2048, 2049, 4100)      # blocks: 1, 1, 1, 2, 8, 9, 15, 512 (one trip), 512, 512 (two trips), 512
N_ITER = 3
STATUSES = (0, R.ST_NO_CONVERGENCE, -1)
FLAGS = (0, 1, 7)

# the classes of a planted DI row
ZEROS, NEG_ZEROS, NEGATIVE, DENORMAL, AT_CAP, NEXT_ABOVE_CAP, ABOVE_CAP, ORDINARY, LAST_SAMPLE, SLOT0, SLOT1, SLOT2, SLOT3 = range(13)


def _cases():
    cases = []
    for k, n in enumerate(N_LIST):
        cases += [(n, NARROW_P[k % len(NARROW_P)]), (n, WIDE_P[k % len(WIDE_P)])]
    cases.append((4100, 256))
    for p in NARROW_P + WIDE_P:
        cases += [(33, p), (2049, p)]
    return sorted(set(cases))


CASES = _cases()


def row_classes(p):
    """The classes a cohort of p samples can hold: a per-lane slot exists when it has a sample (wide cohorts only)."""
    return list(range(LAST_SAMPLE + 1)) + ([SLOT0 + q for q in range(4) if 64 * q < p] if p > 64 else [])


def planted_rho(rng, n, p, shift=0):
    """n x p raw DI rows, the classes dealt round-robin (starting at `shift`) and put in random gene order; returns (rho, labels)."""
    classes = row_classes(p)
    labels = np.array([classes[(g + shift) % len(classes)] for g in range(n)])
    labels = labels[rng.permutation(n)]
    rho = np.zeros((n, p))
    for g, c in enumerate(labels):
        if c == NEG_ZEROS:
            rho[g] = -0.0
        elif c == NEGATIVE:
            rho[g] = -rng.uniform(1e-300, 3.0, p)
        elif c == DENORMAL:
            rho[g, rng.integers(p)] = 5e-324
        elif c == AT_CAP:
            rho[g] = 0.9
        elif c == NEXT_ABOVE_CAP:
            rho[g] = np.nextafter(0.9, 1.0)
        elif c == ABOVE_CAP:
            rho[g] = rng.uniform(0.0, 0.9, p)
            over = rng.random(p) < 0.5
            over[rng.integers(p)] = True
            rho[g, over] = rng.uniform(np.nextafter(0.9, 1.0), 5.0, int(over.sum()))
        elif c == ORDINARY:
            rho[g] = rng.uniform(np.nextafter(0.0, 1.0), 0.9, p)
            rho[g, rng.random(p) < 0.2] = 0.0
            rho[g, rng.integers(p)] = rng.uniform(0.01, 0.9)
        elif c == LAST_SAMPLE:
            rho[g, p - 1] = rng.uniform(0.01, 0.9)
        elif c >= SLOT0:
            q = c - SLOT0
            rho[g, rng.integers(64 * q, min(p, 64 * q + 64))] = rng.uniform(0.01, 2.0)
    return rho, labels


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, '{0}: {1} entries differ, first at {2}: device {3!r}, numpy {4!r}'.format(
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _check_partials(dev_call, terms, n, p, what):
    """Two successive device calls against the fsum and the ordered restatement of the column sums of `terms`."""
    assert np.all(terms >= 0), what
    got, again = dev_call(), dev_call()
    want_fsum, want_ordered = R.fsum_columns(terms), R.ordered_columns(terms)
    print(what, 'max |dev - fsum| / bound:', float(np.max(np.abs(got[:3 * p] - want_fsum[:3 * p]) / np.maximum(R.sum_bound(n, want_fsum[:3 * p]), 5e-324))))
    assert list(got[3 * p:]) == list(want_fsum[3 * p:]), what + ': counts'
    assert np.all(np.abs(got[:3 * p] - want_fsum[:3 * p]) <= R.sum_bound(n, want_fsum[:3 * p])), what + ': sum outside the bound of n additions'
    _same_bits(got, want_ordered, what + ': documented summation order')
    _same_bits(again, got, what + ': second call')
    return want_fsum


def upload_trivial(dev, n, p):
    """n genes of one base (the shortest an upload takes: check_shape wants lengths >= 1), constant positive counts."""
    dev.upload_packed(np.full(n * p, 3.0, np.float32), np.ones(n, np.int64), p)
    return dev


def initial_pass(dev, rng, n, p):
    """dn_init_begin / dn_init_partials / dn_outer_begin_scaled on planted sums whose rho0 sits on either side of 0.1."""
    x = rng.uniform(1.0, 1e6, (n, p))
    est = rng.uniform(0.0, 1e5, (n, p))
    cov = est * rng.uniform(0.3, 1.0, (n, p))                               # ordinary genes: some sample well above 0.1
    kind = rng.permutation(np.arange(n) % 4)
    cov[kind == 1] = (est[kind == 1] + 1.0) * rng.uniform(0.92, 1.3, (int(np.sum(kind == 1)), p))      # low genes
    est[kind >= 2] = cov[kind >= 2] = 9.0                                    # rho0 = 1 - 9 / 10 = 0.09999999999999998 < 0.1: low
    for g in np.flatnonzero(kind == 3):                                      # ... but for one sample just above 0.1: not low
        i = p - 1 if g % 2 else int(rng.integers(p))
        est[g, i] = 9.0 + 1e-9
    rho0 = R.init_rho(est, cov)
    low = rho0.max(axis=1) < 0.1
    if n >= 4:
        assert np.all(low[kind >= 1] == (kind[kind >= 1] < 3)) and rho0[kind == 2].max() < 0.1 < rho0[kind == 3].max(axis=1).min()
    status = rng.choice(STATUSES, n).astype(np.int32)
    dev.init_begin(x)
    dev.debug_plant('est_sums', est)
    dev.debug_plant('cov_sums', cov)
    dev.debug_plant('init_status', status)
    pv = _check_partials(dev.init_partials, R.init_terms(est, cov, status, x), n, p, 'init_partials n={0} p={1}'.format(n, p))
    assert pv[3 * p] == low.sum()
    norm = R.init_norm(pv, p)
    dev.outer_begin_scaled(norm, N_ITER)
    _, _, xw, ran = dev.fetch_outer()
    _same_bits(xw, R.scale_reads(x, norm), 'x_weighted = reads / norm (k_scale_reads)')
    assert not ran.any()


def outer_cycle(dev, rng, n, p, with_avg_first, seen=None):
    """dn_outer_begin, then three outer updates at iter = 0, N_ITER - 1 and N_ITER on freshly planted state, x_weighted carried
    from one to the next as a run carries it; avg_di is given and withheld in turn."""
    xw = rng.uniform(1.0, 1e6, (n, p))
    dev.outer_begin(xw, N_ITER)
    ran = np.zeros((n, N_ITER), dtype=bool)
    for step, it in enumerate((0, N_ITER - 1, N_ITER)):
        what = 'n={0} p={1} iter={2}'.format(n, p, it)
        rho_raw, labels = planted_rho(rng, n, p, shift=n + step)
        if seen is not None:
            seen.update(labels.tolist())
        status, flags = rng.choice(STATUSES, n).astype(np.int32), rng.choice(FLAGS, n).astype(np.int32)
        dev.debug_plant('rho_raw', rho_raw)
        dev.debug_plant('flags', flags)
        dev.debug_plant('iter_status', status)
        got_raw, got_flags = dev.fetch_rows(np.arange(n))                     # the seam wrote what it was given
        _same_bits(got_raw, rho_raw, what + ': planted rho')
        assert np.array_equal(got_flags, flags != 0)

        rho_c = R.clip(rho_raw)
        pv = _check_partials(dev.outer_partials, R.outer_terms(rho_c, xw, status, flags), n, p, 'outer_partials ' + what)
        _same_bits(dev.fetch_outer()[0], rho_c, what + ': clipped rho')

        avg_di, norm = R.derive(pv, p)
        if avg_di is None:                                                    # no untouched gene in a small case: any average will do
            avg_di = rng.uniform(0.05, 0.8, p)
        if (step % 2 == 0) != with_avg_first:
            avg_di = None
        dev.outer_apply(avg_di, norm, it)
        rho, x_adj, xw, ran = R.outer_apply(rho_c, xw, flags, ran, avg_di, norm, it)
        got = dev.fetch_outer()
        _same_bits(got[0], rho, what + ': rho after apply')
        _same_bits(got[1], x_adj, what + ': x_adj = x_w / (1 - rho)')
        _same_bits(got[2], xw, what + ': x_weighted = x_w / norm')
        assert np.array_equal(got[3], ran), what + ': ran_baseline_selection'           # at iter == N_ITER: as it was


@pytest.fixture(scope='module')
def dev():
    d = _lib.Device(0)
    yield d
    d.close()


def test_every_class_of_row_is_planted():
    """Every case of at least 13 genes holds every class its cohort can hold, and the small ones hold them between them."""
    small = set()
    for n, p in CASES:
        rng = np.random.default_rng(1000 * n + p)
        for step in range(3):
            rho, labels = planted_rho(rng, n, p, shift=n + step)
            if n >= 13:
                assert sorted(set(labels)) == row_classes(p), (n, p)
            else:
                small.update(labels.tolist())
            for c, g in ((c, g) for g, c in enumerate(labels)):
                r = rho[g]
                assert {ZEROS: not r.any() and not np.signbit(r).any(), NEG_ZEROS: not r.any() and np.signbit(r).all(), NEGATIVE: (r < 0).all(),
                        DENORMAL: np.count_nonzero(r) == 1 and r.max() == 5e-324, AT_CAP: (r == 0.9).all(),
                        NEXT_ABOVE_CAP: (r == np.nextafter(0.9, 1.0)).all(), ABOVE_CAP: r.max() > 0.9 and r.max() <= 5.0,
                        ORDINARY: 0 < r.max() <= 0.9 and r.min() >= 0, LAST_SAMPLE: np.flatnonzero(r).tolist() == [p - 1]}.get(
                            c, np.count_nonzero(r) == 1 and np.flatnonzero(r)[0] // 64 == c - SLOT0), (n, p, c)
    assert small >= set(range(LAST_SAMPLE + 1))


@pytest.mark.parametrize('n,p', CASES, ids=['n{0}-p{1}'.format(*c) for c in CASES])
def test_outer_update_and_initial_pass(dev, n, p):
    rng = np.random.default_rng(1000 * n + p)
    upload_trivial(dev, n, p)
    initial_pass(dev, np.random.default_rng(7000 * n + p), n, p)
    outer_cycle(dev, rng, n, p, with_avg_first=(n + p) % 2 == 0)


def test_a_larger_cohort_on_the_same_device_sees_no_stale_buffer():
    """A small narrow cohort, then a larger wide one, then a small one again on one Device: every buffer of the outer update
    belongs to the upload, and the block partials of a wide cohort leave nothing behind for a narrow one."""
    d = _lib.Device(0)
    for k, (n, p) in enumerate(((9, 3), (2100, 130), (5, 64), (37, 200), (33, 2))):
        rng = np.random.default_rng(50 + k)
        upload_trivial(d, n, p)
        outer_cycle(d, rng, n, p, with_avg_first=bool(k % 2))
        initial_pass(d, rng, n, p)
        outer_cycle(d, rng, n, p, with_avg_first=not k % 2)
    d.close()
