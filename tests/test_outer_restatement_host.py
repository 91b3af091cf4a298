"""
tests/_outer_restatement.py against the CPU oracle, without a GPU.  oracle.run keeps rho and the scale factors of every outer
iteration; its inputs to the update (raw DI rows, flags, x_weighted) are recovered by replaying its loop line for line with
oracle.baseline_batch, and the replay is first held to that history bit for bit.  The restatement -- per-sample sums over
touched and untouched genes, as the device forms them -- must then give the oracle's elementwise results exactly and its sums
within the bound of a sum of non-negative doubles.
"""
import numpy as np
import pytest

import _outer_restatement as R
from degnorm_amd import synth

SEED, N_GENES, P, ITERS, NMF_ITER = 23, 36, 5, 3, 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope='module')
def replay(oracle):
    covs, reads, _ = synth.synth_dataset(SEED, N_GENES, P, l_min=200, l_max=700)
    covs = list(covs.values())
    x = np.array(reads, dtype=np.float64)
    # genes that no baseline can be found for: the DI row stays 0 and correct_di_scores fills in the average
    for g in (3, 17):
        covs[g] = np.ones_like(covs[g])
    hist = {}
    out = oracle.run(covs, x, degnorm_iter=ITERS, nmf_iter=NMF_ITER, history=hist)

    prm = oracle.make_params(NMF_ITER)
    est_sums, cov_sums, status0 = oracle.ratio_svd_batch(covs)
    rho0 = 1 - (cov_sums / (est_sums + 1))
    low = rho0.max(axis=1) < 0.1
    count_sums = x[low, :].sum(axis=0) if np.any(low) else x.sum(axis=0)
    norm = count_sums / np.median(count_sums)
    steps = [dict(est_sums=est_sums, cov_sums=cov_sums, status=status0, x=x, low=low, norm=norm)]
    xw, scale = x / norm, np.copy(norm)
    assert np.array_equal(_bits(scale), _bits(hist['scale_init']))
    for i in range(ITERS):
        raw, flags, trace, _ = oracle.baseline_batch(covs, scale, prm)
        rho = raw.copy()
        rho[rho > 0.9] = 0.9
        rho[rho < 0.] = 0.
        clipped = rho.copy()
        x_adj = xw / (1 - rho)
        non_bl = rho.max(axis=1) == 0
        avg = None
        if np.sum(non_bl) > 0:
            avg = 1 - (xw.sum(axis=0) / x_adj.sum(axis=0))
            rho[non_bl, :] = avg
        x_adj = xw / (1 - rho)
        norm = x_adj.sum(axis=0) / np.median(x_adj.sum(axis=0))
        steps.append(dict(raw=raw, flags=flags, status=trace[:, 6].copy(), xw=xw, clipped=clipped, avg=avg, rho=rho, x_adj=x_adj,
                          norm=norm, xw_next=xw / norm))
        xw, scale = xw / norm, scale * norm
        assert np.array_equal(_bits(rho), _bits(hist['rho'][i])) and np.array_equal(_bits(scale), _bits(hist['scale'][i]))
        assert np.array_equal(trace, hist['trace'][i])
    assert np.array_equal(_bits(steps[-1]['x_adj']), _bits(out['x_adj'])) and np.array_equal(_bits(xw), _bits(out['x_weighted']))
    return steps, out


def test_the_cohort_has_touched_and_untouched_genes(replay):
    steps, _ = replay
    for s in steps[1:]:
        u = R.untouched(s['clipped'])
        assert 0 < u.sum() < N_GENES and s['avg'] is not None


def test_initial_pass_against_the_oracle(replay):
    s = replay[0][0]
    n = len(s['x'])
    terms = R.init_terms(s['est_sums'], s['cov_sums'], s['status'], s['x'])
    assert np.all(terms >= 0)
    pv, po = R.init_partials(s['est_sums'], s['cov_sums'], s['status'], s['x']), R.init_partials_ordered(s['est_sums'], s['cov_sums'], s['status'], s['x'])
    assert pv[3 * P] == s['low'].sum() and pv[3 * P + 1] == np.sum(s['status'] != 0)
    # whole-number read counts: both sums are exact, and so is everything derived from them
    assert np.array_equal(_bits(pv), _bits(po))
    assert np.array_equal(_bits(pv[P:2 * P]), _bits(s['x'].sum(axis=0)))
    norm = R.init_norm(pv, P)
    assert np.array_equal(_bits(norm), _bits(s['norm']))
    assert np.array_equal(_bits(R.scale_reads(s['x'], norm)), _bits(replay[0][1]['xw']))
    assert np.all(np.abs(po - pv) <= R.sum_bound(n, pv))


def test_outer_update_against_the_oracle(replay):
    steps, out = replay
    ran = np.zeros((N_GENES, ITERS), dtype=bool)
    for i, s in enumerate(steps[1:]):
        n = len(s['xw'])
        rho_c = R.clip(s['raw'])
        assert np.array_equal(_bits(rho_c), _bits(s['clipped']))
        terms = R.outer_terms(rho_c, s['xw'], s['status'], s['flags'])
        assert np.all(terms >= 0)
        pv, po = R.outer_partials(rho_c, s['xw'], s['status'], s['flags']), R.outer_partials_ordered(rho_c, s['xw'], s['status'], s['flags'])
        # counts exact; the ordered sum within the bound of the correctly rounded one; numpy's own (pairwise) sums as well
        u = R.untouched(rho_c)
        want_counts = [u.sum(), np.sum(s['status'] != 0), np.sum(s['status'] == R.ST_NO_CONVERGENCE), np.sum(s['flags'])]
        assert list(pv[3 * P:]) == want_counts and list(po[3 * P:]) == want_counts
        assert np.all(np.abs(po - pv) <= R.sum_bound(n, pv))
        first_adj = s['xw'] / (1 - rho_c)
        for got, ref in ((pv[:P] + pv[P:2 * P], first_adj.sum(axis=0)), (pv[2 * P:3 * P], s['xw'].sum(axis=0))):
            assert np.all(np.abs(got - ref) <= 2 * R.sum_bound(n, ref))
        # avg_di = 1 - W / S and norm = S / median(S): W <= S, so an error of k ulp-sized relative errors in W and S moves
        # avg_di by at most that much absolutely, and norm by twice that relatively (S and the median both carry it)
        avg, norm = R.derive(pv, P)
        tol = (2 * n + 4) * 2.0 ** -53
        assert np.all(np.abs(avg - s['avg']) <= tol)
        assert np.all(np.abs(norm - s['norm']) <= 4 * tol / (1 - 0.9) * s['norm'])
        # with the oracle's own average and norm, the elementwise results are the oracle's bit for bit
        rho, x_adj, xw_next, ran = R.outer_apply(rho_c, s['xw'], s['flags'], ran, s['avg'], s['norm'], i)
        for got, ref in ((rho, s['rho']), (x_adj, s['x_adj']), (xw_next, s['xw_next'])):
            assert np.array_equal(_bits(got), _bits(ref))
    assert np.array_equal(ran, out['ran_baseline_selection'])
    again = R.outer_apply(rho_c, s['xw'], s['flags'], ran, s['avg'], s['norm'], ITERS)[3]        # iter == n_iter: nothing is written
    assert np.array_equal(again, ran)


def test_ordered_sum_is_the_documented_order():
    """The vectorised ordered sum against the order written out gene by gene, at block counts on both sides of a multiple of 8
    and of the 512-block cap, on terms whose sum depends on the order."""
    rng = np.random.default_rng(5)
    for n in (1, 3, 4, 5, 32, 33, 60, 2047, 2049, 4100):
        terms = rng.uniform(0.0, 1.0, (n, 2)) * 10.0 ** rng.integers(-8, 8, (n, 2))
        blocks = min(512, (n + 3) // 4)
        part = []
        for b in range(blocks):
            waves = []
            for w in range(4):
                acc = np.zeros(2)
                for g in range(4 * b + w, n, 4 * blocks):
                    acc = acc + terms[g]
                waves.append(acc)
            part.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
        a = [np.zeros(2) for _ in range(8)]
        for b in range(blocks):
            a[b % 8] = a[b % 8] + part[b]
        want = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))
        got = R.ordered_columns(terms)
        assert np.array_equal(_bits(got), _bits(want)), n
        fs = R.fsum_columns(terms)
        assert np.all(np.abs(got - fs) <= R.sum_bound(n, fs)), n
