"""
Hand-down on the device (csrc/dn_kernels.hpp k_baseline, csrc/dn_api.hip dn_baseline_iteration): a gene of the wide or the narrow
class whose drop loop has shrunk it to the next class's on-chip capacity is parked between two nmf() calls and finished by a second
launch of that class.  Short genes through DN_SPLIT_LEN=600 DN_TINY_LEN=300 DN_HANDDOWN_COLS=400,200 (read at the upload), so that
every class has genes on either side of its boundary; against the CPU oracle (trace, flags and the dropped-bin sequence exact, DI
within rtol 1e-8 / atol 1e-10, the figure the parity tests hold these kernels to) and against the same run with DN_HANDDOWN=0.
Which genes are parked is predicted from the oracle's traces by tests/_handdown_cases.py; tests/test_handdown_host.py asserts on the
CPU that every case below parks genes at all.

Covered:
  sample counts    2, 3, 6, 9, 12 (three classes, every register-tier width of rt_cols), 10, and 13, 16, 17, 24 (no pair class, no
                   register tier: the wide class parks, counts [n, 0, 0]; 17 and 24 on the row solver), each through park and resume;
  parameter sets   (bins, T, min_high_coverage) = (20, 12, 50), (5, 12, 50), (32, 12, 50), (20, 3, 50), (32, 1, 10), hand-down on and off;
  exits            of parked genes: (refined, min_bins), (not_found_fallback, min_bins), (refined, natural) and
                   (not_found_fallback, zero_rowsum), with n0 == L and n0 < L.  The oracle reaches refine_fallback, perfect and
                   value_error on no parked gene of these sets, so no device test holds a continuation into those three;
  bin limit        32 bins (HAND_MAX_BINS, the record full) parks, 33 parks nothing; 33, 20, 5 in a row on one handle;
  x16 = 0          parked genes with counts that are not whole numbers or exceed 65535 (the body that re-reads its counts);
  equality         n <= handdown_cols at n == handdown_cols and at one column more;
  estimates        a want_estimates iteration behind one that parked genes;
  shipped widths   no DN_SPLIT_LEN / DN_TINY_LEN / DN_HANDDOWN_COLS: the receiver's own reg_tier_cols + lds_cols, slots sized for the
                   donor's longest gene, on genes of a few thousand columns.
A parked gene that ends in the not-found fallback reports the donor's rho_fb: bit for bit what the run without hand-down reports.
The base genes hold piecewise-constant ones (synth.pileup_gene) with exact ties between bin means, which the summation order decides
on the device with or without hand-down: where a dropped-bin sequence parts from the oracle's, the two bins' means must agree
within 1e-12 in the oracle's own arithmetic (tests/_handdown_cases.py first_tie_flip), or the test fails.
Each test prints the largest DI error of the parked and of the unparked genes (pytest -s).
"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _handdown_cases as hc                                   # noqa: E402
import test_handdown_host as hh                                # noqa: E402

pytestmark = pytest.mark.gpu

P, T, BINS = 10, 12, 20
SPLIT, TINY, COLS = hc.SPLIT, hc.TINY, hc.COLS
ENV = hc.ENV
SCALES = (np.linspace(0.9, 1.2, P), np.linspace(1.3, 0.8, P))
RTOL_DI, ATOL_DI = 1e-8, 1e-10
HAND_VARS = ('DN_SPLIT_LEN', 'DN_TINY_LEN', 'DN_HANDDOWN_COLS', 'DN_HANDDOWN')


@contextlib.contextmanager
def _environment(env, handdown):
    """The hand-down variables as the next upload is to read them (those not in `env` unset), put back afterwards."""
    old = {k: os.environ.get(k) for k in HAND_VARS}
    for k in HAND_VARS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ['DN_HANDDOWN'] = '1' if handdown else '0'
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(covs, handdown, scales, want_estimates=False, psets=None, env=ENV):
    """One handle: upload, one baseline_iteration per scale vector -- with the parameter set (bins, T, min_high_coverage) of the same
    index in `psets` and with estimates where `want_estimates` (one value, or one per iteration) says so.  Returns per iteration
    (rho, flags, trace, parked per class[, est]) and the hand-down width of every class."""
    from degnorm_amd import _lib
    psets = psets or [(BINS, T, 50)] * len(scales)
    want = want_estimates if isinstance(want_estimates, (list, tuple)) else [want_estimates] * len(scales)
    p = covs[0].shape[0]
    with _environment(env, handdown):
        dev = _lib.Device(0)
        try:
            dev.upload(covs)
            if 'DN_SPLIT_LEN' in env:
                assert dev.split_length() == SPLIT and dev.tiny_length() == hc.tiny_len(p)
            out = []
            for s, (bins, t, mhc), we in zip(scales, psets, want):
                rho, flags, trace = dev.baseline_iteration(s, nmf_iter=t, bins=bins, min_high_coverage=mhc, want_estimates=we)
                res = [rho.copy(), flags.copy(), trace.copy(), [dev.handdown(c)[1] for c in range(3)]]
                if we:
                    res.append([e.copy() for e in dev.fetch_estimates()])
                out.append(res)
            cols = [dev.handdown(c)[0] for c in range(3)]
            return out, cols
        finally:
            dev.close()


@pytest.fixture(scope='module')
def genes():
    return hh.handdown_genes(P)


@pytest.fixture(scope='module')
def oracle_runs(oracle, genes):
    return [oracle.baseline_batch(genes, s, oracle.make_params(nmf_iter=T, bins=BINS)) for s in SCALES]


@pytest.fixture(scope='module')
def runs(genes):
    return {hd: _run(genes, hd, SCALES) for hd in (True, False)}


def _against_oracle(res, ora):
    rho, flags, trace = res[:3]
    rho_o, flags_o, trace_o = ora[:3]
    np.testing.assert_array_equal(trace[:, :7], trace_o[:, :7])
    np.testing.assert_array_equal(flags, flags_o)
    np.testing.assert_allclose(rho, rho_o, rtol=RTOL_DI, atol=ATOL_DI)


def _di_error(rho, rho_o, rows):
    """Largest DI error over the genes `rows`, relative to max(|DI|, 0.01) (below that the tolerance is an absolute one)."""
    rows = sorted(rows)
    if not rows:
        return 0.0
    return float(np.max(np.abs(rho[rows] - rho_o[rows]) / np.maximum(np.abs(rho_o[rows]), 1e-2)))


def _hold_to_oracle(res, ora, parked, want_counts, what, inputs):
    """Everything the device reports for an iteration against the oracle's (rho, flags, trace): counters, flags and the dropped-bin
    sequence exact, DI at the tolerance, the parked counts as predicted.  `parked`: the genes predicted to be parked, per class.
    `inputs` = (oracle, covs, scale, parameter set).  One exception, gene by gene: where the dropped-bin sequences part at two bins
    whose means the oracle's own arithmetic cannot tell apart (hc.first_tie_flip: equal within 1e-12), the summation order decides
     and the rest of that gene's sequence is not compared; its counters, flag and DI still are."""
    rho, flags, trace, counts = res[:4]
    rho_o, flags_o, trace_o = ora[:3]
    moved = set(parked[0]) | set(parked[1])
    rest = set(range(len(rho))) - moved
    print('%s: parked %s, largest DI error parked %.2e unparked %.2e' % (what, counts, _di_error(rho, rho_o, moved), _di_error(rho, rho_o, rest)))
    np.testing.assert_array_equal(trace[:, :7], trace_o[:, :7], err_msg=what)
    np.testing.assert_array_equal(flags, flags_o, err_msg=what)
    oracle, covs, scale, pset = inputs
    for g in np.flatnonzero((trace[:, 8:40] != trace_o[:, 8:40]).any(axis=1)):
        k, gap = hc.first_tie_flip(oracle, covs[g], scale, pset, trace[g, 8:8 + trace[g, 5]], trace_o[g, 8:8 + trace_o[g, 5]])
        print('%s: gene %d (%s) drop %d: device bin %d, oracle bin %d, means apart by %.1e' % (
            what, g, 'parked' if g in moved else 'not parked', k, trace[g, 8 + k], trace_o[g, 8 + k], gap))
        assert gap <= hc.TIE_RTOL, '%s: gene %d drops %s, the oracle %s' % (what, g, trace[g, 8:40].tolist(), trace_o[g, 8:40].tolist())
    np.testing.assert_allclose(rho, rho_o, rtol=RTOL_DI, atol=ATOL_DI, err_msg=what)
    assert counts == want_counts, what


def _carried_bits(on, off, trace_o, parked, what):
    """A parked gene that ends in the not-found fallback reports rho_fb, which its donor computed after the first call and the record
    carried: the same bits as without hand-down, where one class does it all."""
    rows = [g for g in parked[0] + parked[1] if trace_o[g, 3] == hc.EXIT_NOT_FOUND_FALLBACK]
    np.testing.assert_array_equal(on[0][rows], off[0][rows], err_msg=what)
    return len(rows)


def test_handdown_matches_oracle_and_parks_the_predicted_genes(genes, oracle_runs, runs):
    out, cols = runs[True]
    assert cols == [COLS[0], COLS[1], 0]
    lengths = [c.shape[1] for c in genes]
    _against_oracle(out[0], oracle_runs[0])
    want = hh.predicted_parked(lengths, oracle_runs[0][2], BINS, SPLIT, TINY, COLS)
    assert want[0] >= 3 and want[1] >= 3                         # both upper classes hand genes down, and
    assert (oracle_runs[0][2][:, 1] == 1).sum() >= 2             # some genes leave after one call: never parked
    assert out[0][3] == want
    np.testing.assert_array_equal(out[0][2][:, 8:40], oracle_runs[0][2][:, 8:40])     # the dropped-bin sequence, written by two classes


def test_handdown_off_matches_oracle_and_the_run_with_it(oracle_runs, runs):
    off, cols = runs[False]
    _against_oracle(off[0], oracle_runs[0])
    assert off[0][3] == [0, 0, 0]
    np.testing.assert_array_equal(off[0][2][:, :7], runs[True][0][0][2][:, :7])
    np.testing.assert_array_equal(off[0][1], runs[True][0][0][1])


def test_second_iteration_on_the_same_handle(genes, oracle_runs, runs):
    """Other scale factors on the same handle: stale continuation counters or records would show."""
    out, _ = runs[True]
    _against_oracle(out[1], oracle_runs[1])
    lengths = [c.shape[1] for c in genes]
    assert out[1][3] == hh.predicted_parked(lengths, oracle_runs[1][2], BINS, SPLIT, TINY, COLS)


def test_want_estimates_parks_nothing(genes):
    on, _ = _run(genes, True, SCALES[:1], want_estimates=True)
    off, _ = _run(genes, False, SCALES[:1], want_estimates=True)
    assert on[0][3] == [0, 0, 0]
    np.testing.assert_array_equal(on[0][0], off[0][0])
    np.testing.assert_array_equal(on[0][2][:, :8], off[0][2][:, :8])
    for a, b in zip(on[0][4], off[0][4]):
        np.testing.assert_array_equal(a, b)


def test_lone_gene_and_empty_class(oracle, genes):
    """One wide gene alone in its class, no pair class at all: the narrow class's second launch takes one continuation, the narrow
    class itself parks nothing (nobody to hand to), and the launches cope with the empty queues."""
    lengths = [c.shape[1] for c in genes]
    ora = oracle.baseline_batch(genes, SCALES[0], oracle.make_params(nmf_iter=T, bins=BINS))
    wide = [g for g, L in enumerate(lengths) if L > SPLIT and hh.park_call(ora[2][g][0], BINS, ora[2][g][8:8 + ora[2][g][5]], ora[2][g][1], COLS[0])]
    narrow = [g for g, L in enumerate(lengths) if TINY < L <= SPLIT]
    pick = wide[:1] + narrow
    sub = [genes[g] for g in pick]
    out, _ = _run(sub, True, SCALES[:1])
    _against_oracle(out[0], [a[pick] for a in ora[:3]])
    assert out[0][3] == [1, 0, 0]
    # and the other way round: no wide and no narrow gene -- the pair class alone, nothing to receive
    pair = [genes[g] for g, L in enumerate(lengths) if L <= TINY]
    out, _ = _run(pair, True, SCALES[:1])
    _against_oracle(out[0], [a[[g for g, L in enumerate(lengths) if L <= TINY]] for a in ora[:3]])
    assert out[0][3] == [0, 0, 0]


def _widths(p, thresholds=COLS):
    """What dn_handdown reports per class under ENV: a class has a width only if the next one exists."""
    return [thresholds[0], thresholds[1] if p <= 12 else 0, 0]


@pytest.mark.parametrize('p', hc.P_THREE_CLASSES + hc.P_TWO_CLASSES)
def test_sample_counts_and_parameter_sets(oracle, p):
    """Every parameter set in turn on one handle with hand-down, and on one without: the record layout (HAND_INTS integers and
    5 p + 1 doubles per gene) and the restore are a function of p."""
    covs = hc.genes('base', p)
    psets = list(hc.PARAM_SETS)
    scales = [hc.scales(p)] * len(psets)
    both = {}
    for handdown in (True, False):
        out, cols = _run(covs, handdown, scales, psets=psets)
        both[handdown] = out
        assert cols == _widths(p)
        for res, pset in zip(out, psets):
            parked = hc.parked_of(oracle, 'base', p, pset)
            want = [len(v) for v in parked] if handdown else [0, 0, 0]
            if handdown:
                assert want[0] >= 1 and (want[1] >= 1) == (p <= 12) and want[2] == 0
            _hold_to_oracle(res, hc.oracle_run(oracle, 'base', p, pset), parked, want, 'p=%d %s hand-down %s' % (p, pset, 'on' if handdown else 'off'), (oracle, covs, hc.scales(p), pset))
    carried = sum(_carried_bits(on, off, hc.oracle_run(oracle, 'base', p, pset)[2], hc.parked_of(oracle, 'base', p, pset), 'p=%d %s' % (p, pset))
                  for on, off, pset in zip(both[True], both[False], psets))
    assert carried >= 3


@pytest.mark.parametrize('p', (10, 16))
def test_bin_limit(oracle, p):
    """32 bins fill the record's alive[] and park; 33 bins switch hand-down off for that iteration.  Then 33, 20, 5 on one handle:
    a record or a queue count must not survive an iteration that did not use it."""
    covs = hc.genes('base', p)
    for bins_seq in ((32, 33), (33, 20, 5)):
        psets = [(b, 12, 50) for b in bins_seq]
        out, _ = _run(covs, True, [hc.scales(p)] * len(psets), psets=psets)
        for res, pset in zip(out, psets):
            parked = hc.parked_of(oracle, 'base', p, pset) if pset[0] <= 32 else [[], [], []]
            want = [len(v) for v in parked]
            assert (want[0] >= 3) == (pset[0] <= 32)
            ora = hc.oracle_run(oracle, 'base', p, pset)
            if pset[0] == 33:
                assert ora[2][:, 5].max() <= 32 and (ora[2][:, 1] >= 10).sum() >= 3          # the drop loops still run, all drops recorded
            _hold_to_oracle(res, ora, parked, want, 'p=%d bins %s of %s' % (p, pset[0], bins_seq), (oracle, covs, hc.scales(p), pset))


@pytest.mark.parametrize('kind,p', [(k, p) for k in ('fractional', 'deep') for p in hc.P_X16] + list(hc.OTHER_KINDS))
def test_genes_that_reread_their_counts(oracle, kind, p):
    """Parked genes with x16 = 0 -- counts that are not whole numbers (`fractional`) or exceed 65535 (`deep`) take the body without
    packed counts on both sides of the hand-over -- and the `decay` and `holes` generators."""
    covs = hc.genes(kind, p)
    pset = hc.X_PARAMS
    parked = hc.parked_of(oracle, kind, p, pset)
    want = [len(v) for v in parked]
    odd = {g for g, c in enumerate(covs) if not hc.is_x16(c)}
    if kind in ('fractional', 'deep'):
        assert len(odd.intersection(parked[0] + parked[1])) >= 2
    else:
        assert sum(want) >= 1
    both = {}
    for handdown in (True, False):
        out, cols = _run(covs, handdown, [hc.scales(p)], psets=[pset])
        assert cols == _widths(p)
        both[handdown] = out[0]
        _hold_to_oracle(out[0], hc.oracle_run(oracle, kind, p, pset), parked, want if handdown else [0, 0, 0],
                        '%s p=%d hand-down %s' % (kind, p, 'on' if handdown else 'off'), (oracle, covs, hc.scales(p), pset))
    _carried_bits(both[True], both[False], hc.oracle_run(oracle, kind, p, pset)[2], parked, '%s p=%d' % (kind, p))


@pytest.mark.parametrize('p', (10, 16))
def test_threshold_at_equality(oracle, p):
    """n <= handdown_cols: a wide gene whose last call runs on w columns is parked before it at width w and never at w - 1."""
    pset = hc.PARAM_SETS[0]
    pick, k, w = hc.equality_case(oracle, p, pset)
    covs = [hc.genes('base', p)[g] for g in pick]
    ora = [a[pick] for a in hc.oracle_run(oracle, 'base', p, pset)]
    for width, n_parked in ((w, 1), (w - 1, 0)):
        env = dict(ENV, DN_HANDDOWN_COLS='%d,%d' % (width, COLS[1]))
        out, cols = _run(covs, True, [hc.scales(p)], psets=[pset], env=env)
        assert cols == [width, 0, 0]                                # no pair gene among them: the narrow class has nobody to hand to
        parked = [[k] if n_parked else [], [], []]
        assert hh.predicted_parked([c.shape[1] for c in covs], ora[2], pset[0], SPLIT, hc.tiny_len(p), (width, COLS[1])) == [n_parked, 0, 0]
        _hold_to_oracle(out[0], ora, parked, [n_parked, 0, 0], 'p=%d width %d' % (p, width), (oracle, covs, hc.scales(p), pset))


@pytest.mark.parametrize('p', (10, 16))
def test_estimates_after_an_iteration_that_parked(oracle, p):
    """An iteration that parks genes, then one with want_estimates on the same handle: it parks nothing, and its estimates are the
    oracle's -- nothing of the records, the queues or the second launches reaches it."""
    covs = hc.genes('base', p)
    pset = hc.PARAM_SETS[0]
    scales = [hc.scales(p), np.linspace(1.3, 0.8, p)]
    out, _ = _run(covs, True, scales, want_estimates=[False, True], psets=[pset, pset])
    parked = hc.parked_of(oracle, 'base', p, pset)
    _hold_to_oracle(out[0], hc.oracle_run(oracle, 'base', p, pset), parked, [len(v) for v in parked], 'p=%d first iteration' % p, (oracle, covs, scales[0], pset))
    rho_o, flags_o, trace_o, est_o = oracle.baseline_batch(covs, scales[1], oracle.make_params(nmf_iter=pset[1], bins=pset[0]), want_estimates=True)
    assert (trace_o[:, 1] >= 10).sum() >= 3
    _hold_to_oracle(out[1], (rho_o, flags_o, trace_o), [[], [], []], [0, 0, 0], 'p=%d want_estimates' % p, (oracle, covs, scales[1], pset))
    for a, b in zip(out[1][4], est_o):
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-8)


def _decaying_gene(rng, p, L):
    """Deep coverage that half of the samples lose steeply towards the 5' end: the drop loop runs long."""
    env = 1.0 + np.abs(np.sin(np.linspace(0, rng.uniform(0.5, 7), L) + rng.uniform(0, 3)))
    mean = 60.0 * np.outer(rng.lognormal(0, 0.3, p), env)
    for i in range(0, p, 2):
        mean[i] *= np.linspace(rng.uniform(0.02, 0.2), 1.0, L) ** rng.uniform(1.5, 3)
    return rng.poisson(mean).astype(float)


@pytest.mark.parametrize('p', (6, 10, 16))
def test_shipped_thresholds(oracle, p):
    """No override: the class boundaries of class_lengths(p), the receiver's own reg_tier_cols + lds_cols as the width, its slots
    sized for the donor's longest gene.  About four genes per class, the donors' a little longer than the boundary below them and
    strongly degraded; drawn again until the oracle says that every donor class parks one."""
    from degnorm_amd import _lib
    with _environment({}, True):
        dev = _lib.Device(0)
        try:
            dev.upload([np.ones((p, 64))])
            split, tiny = dev.class_lengths(p)
            assert split > 0 and (tiny > 0) == (p <= 12)
            # the widths need all classes in place: genes of the lengths the test will use, flat coverage
            bounds = [split, tiny] if tiny else [split]
            dev.upload([np.ones((p, b + 64)) for b in bounds] + [np.ones((p, bounds[-1] - 64))])
            widths = [dev.handdown(c)[0] for c in range(3)]
        finally:
            dev.close()
    donors = len(bounds)
    assert all(0 < widths[c] < bounds[c] for c in range(donors)) and not any(widths[donors:])
    pset = hc.PARAM_SETS[0]
    scale = hc.scales(p)
    covs = _genes_around(oracle, p, bounds, widths, pset, scale)
    lengths = [c.shape[1] for c in covs]
    assert len(covs) <= 12 and max(lengths) < 2 * split
    ora = oracle.baseline_batch(covs, scale, oracle.make_params(nmf_iter=pset[1], bins=pset[0], min_high_coverage=pset[2]))[:3]
    parked = hc.parked_genes(lengths, ora[2], pset[0], split, tiny, widths)
    want = [len(v) for v in parked]
    assert all(want[c] >= 1 for c in range(donors)) and not any(want[donors:])
    for handdown in (True, False):
        out, cols = _run(covs, handdown, [scale], psets=[pset], env={})
        assert cols == widths
        _hold_to_oracle(out[0], ora, parked, want if handdown else [0, 0, 0], 'p=%d shipped widths %s, hand-down %s' % (p, widths, 'on' if handdown else 'off'),
                        (oracle, covs, scale, pset))


def _genes_around(oracle, p, bounds, widths, pset, scale):
    """Four genes per class for class boundaries `bounds` (wide / narrow[, narrow / pair]): the donors' up to an eighth longer than the
    boundary below them, up to three of each donor class predicted to park at that class's width, and one with flat coverage."""
    donors = len(bounds)
    prm = oracle.make_params(nmf_iter=pset[1], bins=pset[0], min_high_coverage=pset[2])
    rng = np.random.default_rng(700 + p)
    covs = []
    for c in range(donors):
        keep, spare = [], []
        for attempt in range(6):
            pool = [_decaying_gene(rng, p, bounds[c] + int(rng.integers(1, 1 + bounds[c] // 8))) for _ in range(4)]
            trace = oracle.baseline_batch(pool, scale, prm)[2]
            for cov, tr in zip(pool, trace):
                parks = hc.park_call(tr[0], pset[0], tr[8:8 + min(int(tr[5]), 32)], tr[1], widths[c]) is not None
                (keep if parks else spare).append(cov)
            if len(keep) >= 2:
                break
        assert keep, 'no gene of class %d gets as narrow as %d columns' % (c, widths[c])
        covs += keep[:3]
        covs.append(rng.poisson(40.0, size=(p, bounds[c] + 17)).astype(float))        # flat coverage: nothing but Poisson noise to drop
    covs += [_decaying_gene(rng, p, bounds[-1] - int(rng.integers(0, bounds[-1] // 3))) for _ in range(4)]
    return covs
