"""
Hand-down on the device (csrc/dn_kernels.hpp k_baseline, csrc/dn_api.hip dn_baseline_iteration): a gene of the wide or the narrow
class whose drop loop has shrunk it to the next class's on-chip capacity is parked between two nmf() calls and finished by a second
launch of that class.  Short genes through DN_SPLIT_LEN=600 DN_TINY_LEN=300 DN_HANDDOWN_COLS=400,200 (read at the upload), so that
every class has genes on either side of its boundary; against the CPU oracle (trace and flags exact, DI within 1e-5 relative, the
tolerance of bench.py's parity check) and against the same run with DN_HANDDOWN=0.  Which genes are parked is predicted from the
oracle's traces by tests/test_handdown_host.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_handdown_host as hh                                # noqa: E402

pytestmark = pytest.mark.gpu

P, T, BINS = 10, 12, 20
SPLIT, TINY, COLS = 600, 300, (400, 200)
ENV = {'DN_SPLIT_LEN': str(SPLIT), 'DN_TINY_LEN': str(TINY), 'DN_HANDDOWN_COLS': '%d,%d' % COLS}
SCALES = (np.linspace(0.9, 1.2, P), np.linspace(1.3, 0.8, P))
RTOL_DI = 1e-5


def _run(covs, handdown, scales, want_estimates=False):
    """One handle: upload, one baseline_iteration per scale vector.  Returns per iteration (rho, flags, trace, parked per class[, est])."""
    from degnorm_amd import _lib
    old = {k: os.environ.get(k) for k in list(ENV) + ['DN_HANDDOWN']}
    os.environ.update(ENV)
    os.environ['DN_HANDDOWN'] = '1' if handdown else '0'
    try:
        dev = _lib.Device(0)
        try:
            dev.upload(covs)
            assert dev.split_length() == SPLIT and dev.tiny_length() == TINY
            out = []
            for s in scales:
                rho, flags, trace = dev.baseline_iteration(s, nmf_iter=T, bins=BINS, want_estimates=want_estimates)
                res = [rho.copy(), flags.copy(), trace.copy(), [dev.handdown(c)[1] for c in range(3)]]
                if want_estimates:
                    res.append([e.copy() for e in dev.fetch_estimates()])
                out.append(res)
            cols = [dev.handdown(c)[0] for c in range(3)]
            return out, cols
        finally:
            dev.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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
    np.testing.assert_allclose(rho, rho_o, rtol=RTOL_DI, atol=1e-11)


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
