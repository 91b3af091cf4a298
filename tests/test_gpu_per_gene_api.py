"""
The reference's per-gene methods on the float64-input device path (dn_nmf_f64, dn_baseline_selection_f64):
KATs and golden genes generated from the reference, the CPU oracle on non-integer data, error paths, isolation from
the state run() keeps on the device, and the nmf_mpi module twins.
"""
from collections import OrderedDict

import numpy as np
import pytest

from conftest import golden, input_checksum
from degnorm_amd import _lib, nmf_mpi, synth
from degnorm_amd.nmf import GeneNMFOA

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-11
P_SET = (2, 3, 6, 10, 12, 13, 17, 32, 50, 64)


def _lognormal_matrix(rng, p, n):
    """Non-integer p x n data: a rank-one profile times lognormal noise, rows on lognormal scales."""
    a = rng.lognormal(0.0, 1.0, size=p)
    b = rng.lognormal(0.0, 0.7, size=n)
    return np.outer(a, b) * rng.lognormal(0.0, 0.4, size=(p, n))


def test_kat_vs_reference():
    """kat.npz (generated from the reference): nmf() K E and |K|, rank_one_approx K E, ratio_svd; 2 x 2 and n < p included."""
    K = golden('kat')
    mats = []
    for k in range(int(K['n_nmf'])):
        x = K['nmf%d_x' % k]
        mats.append(x)
        m = GeneNMFOA(nmf_iter=int(K['nmf%d_T' % k]))
        Kk, Ek = m.nmf(x, factors=True)
        assert Kk.shape == (x.shape[0], 1) and Ek.shape == (1, x.shape[1])
        np.testing.assert_allclose(Kk.dot(Ek), K['nmf%d_KE' % k], rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(np.abs(Kk).ravel(), K['nmf%d_absK' % k], rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(m.nmf(x), K['nmf%d_KE' % k], rtol=RTOL, atol=1e-9)
        K1, E1 = GeneNMFOA.rank_one_approx(x)
        assert K1.shape == (x.shape[0], 1) and E1.shape == (1, x.shape[1])
        np.testing.assert_allclose(K1.dot(E1), K['nmf%d_r1KE' % k], rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(np.linalg.norm(E1), 1.0, rtol=1e-12)
        np.testing.assert_allclose(m.ratio_svd(x), K['nmf%d_ratio' % k], rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(nmf_mpi.nmf(x, nmf_iter=int(K['nmf%d_T' % k])), K['nmf%d_KE' % k], rtol=RTOL, atol=1e-9)
    for k, est in enumerate(GeneNMFOA().run_ratio_svd_serial(mats)):          # mixed shapes in one call
        np.testing.assert_allclose(est, K['nmf%d_ratio' % k], rtol=RTOL, atol=1e-9)


def test_baseline_selection_on_scaled_float64_vs_golden():
    """genes.npz (the reference's baseline_selection on F = cov / s): the scaled input is not float32-exact."""
    G = golden('genes')
    p = int(G['p'])
    covs = [synth.synth_gene(int(G['seed']), int(g), p, int(G['l_min']), int(G['l_max']))[0] for g in G['gene_ids']]
    assert np.allclose([input_checksum(c) for c in covs], G['checksum'], rtol=0, atol=0)
    F = [c / G['scale'][:, None] for c in covs]
    assert any(np.any(f.astype(np.float32).astype(np.float64) != f) for f in F)
    out = GeneNMFOA(nmf_iter=int(G['nmf_iter'])).run_baseline_selection_serial(F)
    rho = np.vstack([r for r, _, _ in out])
    np.testing.assert_allclose(rho, G['rho'], rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal([f for _, _, f in out], G['flags'])
    for k, (_, e, _) in enumerate(out):
        assert e.shape == F[k].shape
        np.testing.assert_allclose(e.sum(axis=1), G['est_rowsum'][k], rtol=1e-9)
        step = max(1, e.shape[1] // 16)
        np.testing.assert_allclose(e[:, ::step][:, :16], G['est_sample'][k], rtol=1e-9, atol=1e-9)
    out_s = GeneNMFOA(nmf_iter=int(G['nmf_iter']), skip_baseline_selection=True).run_baseline_selection_serial(F)
    assert not any(f for _, _, f in out_s)
    np.testing.assert_allclose(np.vstack([r for r, _, _ in out_s]), G['rho_skip'], rtol=RTOL, atol=ATOL)
    # par_apply_baseline_selection: the clipped rho and the flag column
    m = GeneNMFOA(nmf_iter=int(G['nmf_iter']), degnorm_iter=2)
    m.ran_baseline_selection = np.zeros((len(F), 2), dtype=bool)
    est = m.par_apply_baseline_selection(F, 1)
    np.testing.assert_allclose(m.rho, np.clip(G['rho'], 0.0, 0.9), rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(m.ran_baseline_selection[:, 1], G['flags'])
    assert not m.ran_baseline_selection[:, 0].any() and len(est) == len(F)


def _nmf_cases():
    """(p, n, T) with both halves of the interface: n < p, n <= 12 and beyond, long genes; small T at large p and n."""
    cases = []
    for p in P_SET:
        for n in sorted({2, p - 1, 12, 13, 300, 5000}):
            if n < 2:
                continue
            for T in (0, 1, 20, 100):
                if n >= 5000 and (p >= 17 and T > 1 or T > 20):
                    continue
                if n >= 300 and p >= 32 and T > 20:
                    continue
                cases.append((p, n, T))
    return cases


def test_nmf_rank_one_ratio_vs_oracle(oracle):
    dev = _lib.Device(0)
    rng = np.random.RandomState(20)
    by_pt = {}
    for p, n, T in _nmf_cases():
        by_pt.setdefault((p, T), []).append(n)
    for (p, T), ns in sorted(by_pt.items()):
        mats = [_lognormal_matrix(rng, p, n + int(rng.randint(0, 3)) if n >= 300 else n) for n in ns]
        K, E, est, status = dev.nmf_f64(mats, _lib.NMF, T, want_est=True)     # one launch for the batch
        assert not status.any(), (p, T, status)
        for x, k, e, ke in zip(mats, K, E, est):
            Ko, Eo = oracle.nmf(x, T)
            ref = Ko.dot(Eo)
            tol = 1e-9 * np.abs(ref).max()
            np.testing.assert_allclose(np.outer(k, e), ref, rtol=RTOL, atol=tol, err_msg=str((p, x.shape[1], T)))
            np.testing.assert_allclose(ke, ref, rtol=RTOL, atol=tol)
            np.testing.assert_allclose(np.abs(k), np.abs(Ko.ravel()), rtol=RTOL, atol=tol)
        if T == 0:
            K1, E1, _, st1 = dev.nmf_f64(mats, _lib.NMF_RANK_ONE, 0)
            _, _, est_r, st_r = dev.nmf_f64(mats, _lib.NMF_RATIO, 0, want_est=True)
            assert not st1.any() and not st_r.any()
            for x, k, e, r in zip(mats, K1, E1, est_r):
                Ko, Eo = oracle.rank_one(x)
                np.testing.assert_allclose(np.outer(k, e), Ko.dot(Eo), rtol=RTOL, atol=1e-9 * np.abs(x).max())
                np.testing.assert_allclose(r, oracle.ratio_svd(x), rtol=RTOL, atol=1e-9 * np.abs(x).max())
    dev.close()


def _scaled_genes(p, n_genes, l_min, l_max, seed):
    rng = np.random.RandomState(seed)
    s = rng.lognormal(0.0, 0.3, size=p)
    return [synth.synth_gene(seed, g, p, l_min, l_max)[0] / s[:, None] for g in range(n_genes)]


@pytest.mark.parametrize('p', P_SET)
def test_baseline_selection_vs_oracle(oracle, p):
    """Non-integer genes, full trace; the block path (long active matrices) and nmf_rows (down-sampled, <= 12 columns)."""
    dev = _lib.Device(0)
    T = 100 if p < 32 else 20
    genes = _scaled_genes(p, 4 if p < 32 else 2, 200, 1500 if p < 32 else 400, 100 + p)
    cases = [dict(downsample_rate=1, min_high_coverage=50, ds=None)]
    rate = min(g.shape[1] for g in genes) // 11                                # ~ 11 sampled columns per gene
    ds = np.random.RandomState(p).randint(0, rate, size=len(genes))
    cases.append(dict(downsample_rate=rate, min_high_coverage=2, ds=ds))
    for c in cases:
        rho, flags, trace, est = dev.baseline_selection_f64(genes, nmf_iter=T, min_high_coverage=c['min_high_coverage'],
                                                            downsample_rate=c['downsample_rate'], ds_start=c['ds'], want_est=True)
        for k, F in enumerate(genes):
            r_o, e_o, f_o, t_o = oracle.baseline_selection(F, ds_start=-1 if c['ds'] is None else int(c['ds'][k]), nmf_iter=T,
                                                           min_high_coverage=c['min_high_coverage'],
                                                           downsample_rate=c['downsample_rate'])
            np.testing.assert_array_equal(trace[k, :7], t_o[:7], err_msg=str((p, k, c['downsample_rate'])))
            np.testing.assert_array_equal(trace[k, 8:40], t_o[8:40])
            assert flags[k] == f_o
            np.testing.assert_allclose(rho[k], r_o, rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(est[k], e_o, rtol=RTOL, atol=1e-9 * np.abs(F).max())
    dev.close()


def test_downsampled_class_method_draws_like_the_reference(oracle):
    """downsample_rate > 1: the start offsets come from np.random in gene order (nmf.py:422)."""
    genes = _scaled_genes(10, 5, 600, 1200, 7)
    np.random.seed(11)
    ds = [np.random.choice(50) for _ in genes]
    np.random.seed(11)
    out = GeneNMFOA(downsample_rate=50, nmf_iter=30).run_baseline_selection_serial(genes)
    for F, d, (rho, est, ran) in zip(genes, ds, out):
        r_o, e_o, f_o, _ = oracle.baseline_selection(F, ds_start=int(d), nmf_iter=30, downsample_rate=50)
        np.testing.assert_allclose(rho, r_o, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(est, e_o, rtol=RTOL, atol=1e-9 * np.abs(F).max())
        assert ran == f_o


def test_error_paths_leave_the_device_usable():
    m = GeneNMFOA(nmf_iter=10)
    x = _lognormal_matrix(np.random.RandomState(1), 4, 40)
    good = m.nmf(x)
    with pytest.raises(_lib.DegnormAmdError, match='ArpackError'):
        m.nmf(np.zeros((3, 10)))
    with pytest.raises(_lib.DegnormAmdError, match='ArpackError'):
        GeneNMFOA.rank_one_approx(np.zeros((5, 3)))
    with pytest.raises(ValueError):
        m.nmf(x[:, :1])
    with pytest.raises(ValueError):
        m.ratio_svd(x[:1, :])
    with pytest.raises(ValueError):
        GeneNMFOA().baseline_selection(x[:1, :])
    with pytest.raises(_lib.DegnormAmdError, match='outside'):
        m.nmf(np.ones((65, 10)))
    with pytest.raises(_lib.DegnormAmdError, match='outside'):
        GeneNMFOA().baseline_selection(np.ones((65, 300)))
    with pytest.raises(_lib.DegnormAmdError):                                 # one bad matrix fails the batch, named
        m.run_ratio_svd_serial([x, np.zeros_like(x)])
    np.testing.assert_array_equal(m.nmf(x), good)                              # the same Device, still working
    rho, est, ran = m.baseline_selection(np.zeros((4, 300)))                   # no coverage: the defaults, not an error
    assert not rho.any() and not ran and np.array_equal(est, np.zeros((4, 300)))


def test_per_gene_calls_do_not_touch_run_state():
    p, n_genes = 6, 24
    cfg_seed = 31
    covs = [synth.synth_gene(cfg_seed, g, p, 200, 1500)[0] for g in range(n_genes)]
    names = ['g%d' % g for g in range(n_genes)]
    reads = np.random.RandomState(3).poisson(200.0, size=(n_genes, p)).astype(float) + 1.0
    m = GeneNMFOA(degnorm_iter=2, nmf_iter=20)
    m.run(OrderedDict(zip(names, covs)), reads)
    pick = names[::5]
    before = [e.copy() for e in m.estimates_for(pick)]
    outer = getattr(m._dev, '_n_iter', None) is not None                      # the outer state lives on the device
    state_before = [a.copy() for a in m._dev.fetch_outer()] if outer else []
    rows_before = [a.copy() for a in m._dev.fetch_rows(np.arange(n_genes))]
    rho_host = m.rho.copy()
    rng = np.random.RandomState(4)
    m.nmf(_lognormal_matrix(rng, 9, 700), factors=True)
    m.ratio_svd(_lognormal_matrix(rng, 3, 5000))
    m.run_baseline_selection_serial(_scaled_genes(p, 5, 300, 3000, 8))
    assert m._dev is m._engine.dev                                             # the run's Device did the work
    after = m.estimates_for(pick)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(state_before, m._dev.fetch_outer() if outer else []):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(rows_before, m._dev.fetch_rows(np.arange(n_genes))):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(m.rho, rho_host)


def test_module_twins_match_the_class():
    genes = _scaled_genes(6, 6, 300, 2000, 12)
    cls_out = GeneNMFOA(nmf_iter=40, min_high_coverage=20).run_baseline_selection_serial(genes)
    for F, (rho, est, ran) in zip(genes, cls_out):
        e2, r2, f2 = nmf_mpi.baseline_selection(F, nmf_iter=40)                # min_high_coverage defaults to 20 here
        np.testing.assert_array_equal(r2, rho)
        np.testing.assert_array_equal(e2, est)
        assert f2 == ran
    x = _lognormal_matrix(np.random.RandomState(2), 5, 90)
    K1, E1 = nmf_mpi.rank_one_approx(x)
    K2, E2 = GeneNMFOA.rank_one_approx(x)
    np.testing.assert_array_equal(K1.dot(E1), K2.dot(E2))
    np.testing.assert_array_equal(nmf_mpi.ratio_svd(x), GeneNMFOA().ratio_svd(x))
    np.testing.assert_array_equal(nmf_mpi.run_ratio_svd_serial([x, x[:, :7]])[1], GeneNMFOA().ratio_svd(x[:, :7]))
    Kf, Ef = nmf_mpi.nmf(x, factors=True, nmf_iter=15)
    np.testing.assert_allclose(Kf.dot(Ef), GeneNMFOA(nmf_iter=15).nmf(x), rtol=1e-13)
