"""
Hand-down of a gene to the next narrower class (csrc/dn_kernels.hpp k_baseline, csrc/dn_api.hip dn_baseline_iteration): which nmf()
call of a gene is the first that the donor class does NOT make, restated in Python from n0, bins, the dropped-bin sequence and the
class's threshold (tests/_handdown_cases.py), and checked against the CPU oracle's traces.  tests/test_gpu_handdown.py imports the
restatement to predict how many genes each class parks.

The tests below are the CPU preconditions of tests/test_gpu_handdown.py, so that no device test passes while it exercises nothing.
Covered, all from the oracle:
  sample counts    2, 3, 6, 9, 12 (wide, narrow and pair class; every register-tier width of rt_cols), 10, and 13, 16, 17, 24 (no pair
                   class, no register tier; 17 and 24 on the row solver);
  parameter sets   (bins, T, min_high_coverage) = (20, 12, 50), (5, 12, 50), (32, 12, 50), (20, 3, 50), (32, 1, 10);
  parked counts    every donor class (wide for every p, narrow for p <= 12) parks 3 to 13 genes per set, at least 1 in the T = 1 set;
                   no gene drops more than the 32 bins that trace[8:40] holds; no status is non-zero;
  exits            parked genes end in (refined, min_bins), (not_found_fallback, min_bins), (refined, natural) and
                   (not_found_fallback, zero_rowsum), with n0 == L and with n0 < L; zero_rowsum at p = 16, 17 and 24;
  x16 = 0          parked genes whose counts are not whole numbers (`fractional`) or exceed 65535 (`deep`);
  equality         a wide gene parks at threshold = the width of its last call and not at one column less.
The oracle reaches the exits refine_fallback, perfect and value_error on NO parked gene of these sets (the base genes, `deep`,
`fractional`, `decay`, `holes`): they are asserted absent here, so that a generator that starts to reach one is noticed and the device
tests can be extended to it.
"""
import time

import numpy as np
import pytest

import _handdown_cases as hc
from _handdown_cases import call_widths, park_call, gene_class, predicted_parked, handdown_genes      # noqa: F401  (test_gpu_handdown.py)


def test_call_widths_bins():
    assert call_widths(900, 20, [0, 0]) == [900, 855, 810]
    assert call_widths(301, 20, [18, 0]) == [301, 288, 272]          # 19 bins of 16, the last one of 13 columns
    assert park_call(900, 20, [0] * 16, 17, 400) == 12                 # 900 - 45 k <= 400 from k = 12 on
    assert park_call(900, 20, [0] * 16, 12, 400) is None               # the call at that width is never made
    assert park_call(900, 20, [], 1, 400) is None                      # one call: never parked
    assert park_call(350, 20, [0], 2, 400) == 1                        # below the threshold from the start: parked before the second call
    assert park_call(900, 20, [0] * 16, 17, 0) is None


def test_widths_agree_with_the_oracle_traces(oracle):
    covs = handdown_genes()
    scale = np.linspace(0.9, 1.2, 10)
    rho, flags, trace, _ = oracle.baseline_batch(covs, scale, oracle.make_params(nmf_iter=12))
    many = 0
    for tr in trace:
        if tr[1] == 0:
            continue
        w = call_widths(tr[0], 20, tr[8:8 + tr[5]])
        assert tr[5] <= 32 and len(w) >= tr[1]
        assert sum(w[:tr[1]]) == tr[2]                                 # the columns summed over the gene's calls
        many += tr[1] >= 10
    assert many >= 10 and (trace[:, 1] == 1).sum() >= 2
    lengths = [c.shape[1] for c in covs]
    parked = predicted_parked(lengths, trace, 20, 600, 300, (400, 200))
    assert parked[0] >= 3 and parked[1] >= 3 and parked[2] == 0


@pytest.mark.parametrize('p', (2, 10, 16))
def test_bin_means_restate_the_oracles_drops(oracle, p):
    """hc.bin_means, which the device tests use to tell an exact tie between two bins from a wrong drop: its first maximum is the bin
    the oracle drops, and a sequence that starts with another bin is reported with the gap between the two means."""
    pset = hc.PARAM_SETS[2]
    covs = hc.genes('base', p)
    trace = hc.oracle_run(oracle, 'base', p, pset)[2]
    steps = 0
    for g in range(0, len(covs), 2):                                  # every other gene: synth_gene and pileup_gene draws alike
        drops = trace[g, 8:8 + trace[g, 5]]
        for k in range(0, len(drops), 5):
            means = hc.bin_means(oracle, covs[g], hc.scales(p), pset, drops[:k])
            assert int(np.argmax(means)) == drops[k], (g, k)
            steps += 1
        assert hc.first_tie_flip(oracle, covs[g], hc.scales(p), pset, drops, drops) is None
        if len(drops) >= 2 and drops[0] != drops[1]:
            k, gap = hc.first_tie_flip(oracle, covs[g], hc.scales(p), pset, [drops[1]] + list(drops[1:]), drops)
            assert k == 0 and (gap > hc.TIE_RTOL or drops[1] > drops[0])        # another bin is no tie (or a later one of equal mean)
    assert steps >= 20


@pytest.mark.parametrize('p', hc.P_ALL)
def test_every_donor_class_parks_genes_in_every_parameter_set(oracle, p):
    lengths = [c.shape[1] for c in hc.genes('base', p)]
    for pset in hc.PARAM_SETS:
        bins, T, mhc = pset
        rho, flags, trace = hc.oracle_run(oracle, 'base', p, pset)
        secs = hc.ORACLE_SECONDS[('base', p, pset, None)]
        if secs >= 0.5:                                                # a busy machine: the faster of two runs
            t0 = time.perf_counter()
            oracle.baseline_batch(hc.genes('base', p), hc.scales(p), oracle.make_params(nmf_iter=T, bins=bins, min_high_coverage=mhc))
            secs = min(secs, time.perf_counter() - t0)
        assert secs < 0.5                                              # the device tests wait for this batch: it stays cheap
        assert not trace[:, 6].any()                                   # no status: the reference raises on none of these genes
        assert trace[:, 5].max() <= 25                                 # every drop is in trace[8:40]
        for tr in trace:
            if tr[1]:
                assert sum(call_widths(tr[0], bins, tr[8:8 + tr[5]])[:tr[1]]) == tr[2]
        parked = predicted_parked(lengths, trace, bins, hc.SPLIT, hc.tiny_len(p), hc.COLS)
        for c in (0, 1, 2):
            if c not in hc.donor_classes(p):
                assert parked[c] == 0
            elif T == 1:
                assert 1 <= parked[c] <= 13, (pset, parked)
                assert parked[c] >= 3 or (p == 2 and c == 1), (pset, parked)
            else:
                assert 3 <= parked[c] <= 13, (pset, parked)


BASE_CASES = [('base', p, pset) for p in hc.P_ALL for pset in hc.PARAM_SETS]                          # what the device tests run
X_CASES = [(kind, p, hc.X_PARAMS) for kind in ('fractional', 'deep') for p in hc.P_X16] + [(kind, p, hc.X_PARAMS) for kind, p in hc.OTHER_KINDS]


def _parked_exits(oracle, cases):
    """(exit, loop reason, n0 == L) of every parked gene -> the (kind, p, parameter set) that reach it."""
    seen = {}
    for kind, p, pset in cases:
        lengths = [c.shape[1] for c in hc.genes(kind, p)]
        trace = hc.oracle_run(oracle, kind, p, pset)[2]
        for gs in hc.parked_of(oracle, kind, p, pset):
            for g in gs:
                key = (int(trace[g, 3]), int(trace[g, 4]), bool(trace[g, 0] == lengths[g]))
                seen.setdefault(key, set()).add((kind, p, pset))
    return seen


def test_exits_of_parked_genes(oracle):
    base = _parked_exits(oracle, BASE_CASES)
    pairs = {k[:2] for k in base}
    assert pairs == {(hc.EXIT_REFINED, hc.LOOP_MIN_BINS), (hc.EXIT_NOT_FOUND_FALLBACK, hc.LOOP_MIN_BINS),
                     (hc.EXIT_REFINED, hc.LOOP_NATURAL), (hc.EXIT_NOT_FOUND_FALLBACK, hc.LOOP_ZERO_ROWSUM)}, sorted(pairs)
    assert {k[2] for k in base} == {True, False}                       # estimates as wide as the gene, and re-expanded ones
    # the other generators reach no further exit: none of refine_fallback, perfect and value_error on any parked gene
    assert {k[:2] for k in _parked_exits(oracle, X_CASES)} <= pairs
    zero = set()
    for k, where in base.items():
        if k[1] == hc.LOOP_ZERO_ROWSUM:
            zero |= where
    assert {p for _, p, _ in zero} >= {16, 17, 24}
    assert ('base', 16, (20, 12, 50)) in zero


@pytest.mark.parametrize('p', hc.P_X16)
def test_parked_genes_with_counts_that_are_not_whole(oracle, p):
    covs = hc.genes('fractional', p)
    frac = {g for g, c in enumerate(covs) if not hc.is_x16(c)}
    assert len(frac) == len(hc.X_LENGTHS) * hc.X_DRAWS               # every generated gene; the pair genes that go with them are whole
    assert all(np.array_equal(c, c.astype(np.float32)) for c in covs)
    parked = hc.parked_of(oracle, 'fractional', p, hc.X_PARAMS)
    assert len(frac.intersection(parked[0] + parked[1])) >= 2


@pytest.mark.parametrize('p', hc.P_X16)
def test_parked_genes_with_counts_beyond_16_bits(oracle, p):
    covs = hc.genes('deep', p)
    assert all(np.array_equal(c, c.astype(np.float32)) for c in covs)
    big = {g for g, c in enumerate(covs) if c.max() > 65535.0}
    assert not any(hc.is_x16(covs[g]) for g in big)
    parked = hc.parked_of(oracle, 'deep', p, hc.X_PARAMS)
    for c in hc.donor_classes(p):
        assert len(big.intersection(parked[c])) >= 3, c


@pytest.mark.parametrize('kind,p', hc.OTHER_KINDS)
def test_decay_and_holes_park_genes(oracle, kind, p):
    assert sum(len(v) for v in hc.parked_of(oracle, kind, p, hc.X_PARAMS)) >= 1


@pytest.mark.parametrize('p', (10, 16))
def test_equality_edge(oracle, p):
    pset = hc.PARAM_SETS[0]
    pick, k, w = hc.equality_case(oracle, p, pset)
    covs = hc.genes('base', p)
    lengths = [covs[g].shape[1] for g in pick]
    trace = hc.oracle_run(oracle, 'base', p, pset)[2][pick]
    assert lengths[k] > hc.SPLIT and trace[k, 1] >= 2 and len(pick) >= 2
    tr = trace[k]
    assert park_call(tr[0], pset[0], tr[8:8 + tr[5]], tr[1], w) == tr[1] - 1          # parked before its last call
    assert park_call(tr[0], pset[0], tr[8:8 + tr[5]], tr[1], w - 1) is None
    assert predicted_parked(lengths, trace, pset[0], hc.SPLIT, hc.tiny_len(p), (w, hc.COLS[1])) == [1, 0, 0]
    assert predicted_parked(lengths, trace, pset[0], hc.SPLIT, hc.tiny_len(p), (w - 1, hc.COLS[1])) == [0, 0, 0]
