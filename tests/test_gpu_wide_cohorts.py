"""
Wide cohorts on the device: 65 to 256 samples on the kernel family gen_wide (csrc/dn_generic.hip compiled with DN_GEN_WIDE=1:
gen_wide::k_baseline_gen, gen_wide::k_ratio_svd_wide, the estimates kernel with the scale factors by pointer) and the wide
instantiation (four samples per lane) of the outer-update kernels of csrc/dn_outer.hip, against the CPU oracle (which has no
cap on p).  Tolerances are those of tests/test_gpu_parity.py.  The sample counts: 65 is one past a wavefront, 96 a partly filled second one, 128 / 129 the boundary
between two and three, 200 a ragged fourth, 256 the ceiling where every `tid < p` thread is live.
"""
from collections import OrderedDict

import numpy as np
import pytest

from degnorm_amd import synth

pytestmark = pytest.mark.gpu

# One kernel serves every regime of a wide cohort: `tid < p` needs its 256 threads, so the one-wave routine (nmf_rows with
# R = ceil(p / 64) samples per lane) runs in wave 0 of this kernel and there is no 64-thread family of its own to name.
WIDE_KERNEL = 'gen_wide::k_baseline_gen'
TRACE_COLS = [0, 1, 2, 3, 5, 6]


def _check_iteration(device, oracle, covs, scale, ds_start=None, **prm):
    rho, flags, trace = device.baseline_iteration(scale, want_estimates=True, ds_start=ds_start, **prm)
    est = device.fetch_estimates()
    rho_o, flags_o, trace_o, est_o = oracle.baseline_batch(covs, scale, oracle.make_params(**prm), ds_start=ds_start, want_estimates=True)
    assert not trace_o[:, 6].any()
    np.testing.assert_array_equal(trace[:, TRACE_COLS], trace_o[:, TRACE_COLS])
    np.testing.assert_array_equal(flags, flags_o)
    np.testing.assert_allclose(rho, rho_o, rtol=1e-8, atol=1e-10)
    for a, b in zip(est, est_o):
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-8)
    return trace


def _edge_shapes(p, reduced):
    rng = np.random.default_rng(100 + p)
    if reduced:
        covs = [synth.synth_gene(9, g, p, 60, 400)[0] for g in range(3)]
        covs += [rng.poisson(30, size=(p, L)).astype(float) for L in (2, 65, 257)]
    else:
        covs = [synth.synth_gene(9, g, p, 60, 900)[0] for g in range(10)]
        covs += [rng.poisson(30, size=(p, L)).astype(float) for L in (2, 3, 5, 51, 64, 65, 257)]    # tiny and boundary lengths
    covs.append(np.zeros((p, 40)))                                                                   # all-zero gene
    covs.append(np.tile(np.arange(1, 301, dtype=float), (p, 1)))                                     # exactly rank 1
    return covs


@pytest.mark.parametrize('p', [65, 96, 129, 200, 256])
def test_plain_regime_edge_shapes_vs_oracle(device, oracle, p):
    """Ragged, tiny, all-zero, rank-1 and single-gene inputs through every exit of baseline selection; the reduced shape set and
    two parameter sets at 200 and 256 samples, where the oracle's p x p eigen-solves set the cost."""
    reduced = p >= 200
    covs = _edge_shapes(p, reduced)
    scale = np.linspace(0.9, 1.2, p)
    sets = ((20, 12, 50, False), (5, 3, 2, False), (33, 1, 10, True))
    for bins, T, mhc, skip in (sets[1:] if reduced else sets):
        device.upload(covs)
        assert device.class_kernel_name(0) == WIDE_KERNEL
        _check_iteration(device, oracle, covs, scale, nmf_iter=T, bins=bins, min_high_coverage=mhc, skip_baseline_selection=skip)
    device.upload(covs[:1])                                                                          # a single gene
    rho1, _, _ = device.baseline_iteration(scale, nmf_iter=12)
    np.testing.assert_allclose(rho1[0], oracle.baseline_batch(covs[:1], scale, oracle.make_params(nmf_iter=12))[0][0], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize('p', [65, 129, 256])
def test_ratio_svd_sums_vs_oracle(device, oracle, p):
    """The initial pass (gen_wide::k_ratio_svd_wide: Gram matrix on the fp64 matrix cores in 32-column chunks, block-wide power
    iteration, one pass for the sums); gene lengths that leave a chunk partly filled or barely started, and a zero sample."""
    rng = np.random.default_rng(41 + p)
    covs = [synth.synth_gene(41, g, p, 300, 4000)[0] for g in range(8)]
    covs.append(np.vstack([np.zeros((1, 500)), np.random.default_rng(5).poisson(20, size=(p - 1, 500))]).astype(float))   # a zero sample
    covs += [rng.poisson(25, size=(p, L)).astype(float) for L in (2, 3, 15, 16, 17, 63, 65)]
    device.upload(covs)
    est, cov, status = device.ratio_svd_sums()
    assert device.init_kernel_name() == 'gen_wide::k_ratio_svd_wide'
    est_o, cov_o, status_o = oracle.ratio_svd_batch(covs)
    assert not status.any() and not status_o.any()
    np.testing.assert_allclose(cov, cov_o, rtol=1e-14)
    np.testing.assert_allclose(est, est_o, rtol=1e-10, atol=1e-7)


@pytest.mark.parametrize('p,rate,genes', [(96, 500, 60), (256, 500, 20), (130, 150, 30)])
def test_downsampled_regime_vs_oracle(oracle, p, rate, genes):
    """Take-every `rate`: active matrices of 1 .. 12 columns (rate 500) and up to 33 (rate 150), fewer columns than samples, with
    the drop loop.  Up to 12 columns go to nmf_rows<n, SAFE, R> where that instantiation exists (R = 2 at p = 96: every n but 9;
    R = 3 at p = 130: n <= 6; R = 4 at p = 256: n <= 5), the others and everything wider to the block-wide nmf_gen: all three cases
    mix the two routines inside one gene's drop loop."""
    from degnorm_amd import _lib
    rng = np.random.default_rng(1000 + p + rate)
    covs, offs = [], []
    for k in range(genes):
        L = int(rng.integers(rate + 1, 12 * rate + 1)) if rate != 150 else int(rng.integers(rate + 1, 5001))
        env = 20.0 + 60.0 * np.abs(np.sin(np.linspace(0, rng.uniform(1, 5), L)))
        deg = np.ones((p, L))
        for i in range(p):
            if rng.random() < 0.4:
                deg[i] = np.linspace(rng.uniform(0.3, 0.9), 1.0, L)
        covs.append(rng.poisson(np.outer(rng.lognormal(0, 0.4, p), env) * deg).astype(float))
        offs.append(int(rng.integers(0, rate)))
    offs = np.asarray(offs, dtype=np.int64)
    scale = np.linspace(0.9, 1.1, p)
    dev = _lib.Device(0)
    try:
        dev.hint_downsample(rate)
        dev.upload(covs)
        assert dev.class_kernel_name(0) == WIDE_KERNEL
        trace = _check_iteration(dev, oracle, covs, scale, ds_start=offs, nmf_iter=30, min_high_coverage=2, downsample_rate=rate)
        assert trace[:, 0].min() >= 0 and trace[:, 0].max() <= (12 if rate != 150 else 34)
        assert trace[:, 5].sum() > 0                                        # the drop loop ran
    finally:
        dev.close()


def _cohort_70():
    p = 70
    rng = np.random.default_rng(7070)
    covs = [synth.synth_gene(70, g, p, 200, 1500)[0] for g in range(24)]
    reads = rng.poisson(np.vstack([c.sum(axis=1) / 50.0 + 5.0 for c in covs])).astype(float)
    return p, covs, reads


def test_whole_run_and_outer_update_vs_oracle(oracle):
    """GeneNMFOA.fit on 70 samples against the oracle's run, then the same cohort through ShardedNMFOA with the outer update on the
    device (the wide k_init_partials / k_outer_partials / k_outer_reduce / k_outer_apply) and on the host."""
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd.nmf_mpi import ShardedNMFOA, LocalComm
    p, covs, reads = _cohort_70()
    ref = oracle.run(covs, reads, degnorm_iter=2, nmf_iter=10, want_estimates=True)
    m = GeneNMFOA(degnorm_iter=2, nmf_iter=10)
    est = m.fit(OrderedDict(('gene_%03d' % g, c) for g, c in enumerate(covs)), reads)
    np.testing.assert_array_equal(m.ran_baseline_selection, ref['ran_baseline_selection'])
    np.testing.assert_allclose(m.rho, ref['rho'], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(m.x_adj, ref['x_adj'], rtol=1e-8)
    np.testing.assert_allclose(m.scale_factors, ref['scale_factors'], rtol=1e-8)
    np.testing.assert_allclose(m.x_weighted, ref['x_weighted'], rtol=1e-8)
    est = list(est.values()) if isinstance(est, dict) else est
    for a, b in zip(est, ref['estimates']):
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-8)
    out = []
    for on_device in (True, False):
        eng = ShardedNMFOA(comm=LocalComm(), device=0, degnorm_iter=2, nmf_iter=10)
        eng.device_outer = on_device
        eng.load(covs, reads)
        eng.run(want_estimates=False)
        assert eng._device_outer == on_device
        out.append(eng)
        np.testing.assert_allclose(eng.rho, ref['rho'], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(eng.x_adj, ref['x_adj'], rtol=1e-8)
        np.testing.assert_allclose(eng.x_weighted, ref['x_weighted'], rtol=1e-8)
        np.testing.assert_allclose(eng.scale_factors, ref['scale_factors'], rtol=1e-8)
        np.testing.assert_array_equal(eng.ran_baseline_selection, ref['ran_baseline_selection'])
    np.testing.assert_allclose(out[0].rho, out[1].rho, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(out[0].x_adj, out[1].x_adj, rtol=1e-12)


def _cohort_200():
    p = 200
    rng = np.random.default_rng(200)
    covs = [synth.synth_gene(9, g, p, 60, 400)[0] for g in range(9)]
    reads = rng.poisson(np.vstack([c.sum(axis=1) / 50.0 + 5.0 for c in covs])).astype(float)
    return p, covs, reads


def test_outer_update_with_four_samples_per_lane():
    """The wide outer-update kernels with all four per-lane slots live (p = 200: samples 128 .. 199 in slots 2 and 3, the tail of
    k_outer_reduce<4> beyond p): the device's update against the host's on the same sweeps."""
    from degnorm_amd.nmf_mpi import ShardedNMFOA, LocalComm
    p, covs, reads = _cohort_200()
    out = []
    for on_device in (True, False):
        eng = ShardedNMFOA(comm=LocalComm(), device=0, degnorm_iter=2, nmf_iter=3)
        eng.device_outer = on_device
        eng.load(covs, reads)
        eng.run(want_estimates=False)
        assert eng._device_outer == on_device
        out.append(eng)
    for name in ('rho', 'x_adj', 'x_weighted', 'scale_factors'):
        np.testing.assert_allclose(getattr(out[0], name), getattr(out[1], name), rtol=1e-12, atol=1e-14)
    np.testing.assert_array_equal(out[0].ran_baseline_selection, out[1].ran_baseline_selection)
    assert np.isfinite(out[0].rho).all() and out[0].rho.shape == (9, p)


def _libcomm_worker_200(out_q):
    # no torch in this process: the library binds librccl by itself, the communicator lives in the handle
    from degnorm_amd.nmf_mpi import ShardedNMFOA, LocalComm
    p, covs, reads = _cohort_200()
    eng = ShardedNMFOA(comm=LocalComm(), device=0, degnorm_iter=2, nmf_iter=3)
    eng.load(covs, reads)
    eng.attach_library_comm()
    probe = eng.dev.comm_allreduce(np.arange(3 * 256 + 4, dtype=np.float64))      # DN_COMM_MAX_DOUBLES
    try:
        eng.dev.comm_allreduce(np.zeros(3 * 256 + 5))
        refused = False
    except ValueError:
        refused = True
    eng.run(want_estimates=False)
    out_q.put(dict(rho=eng.rho, x_adj=eng.x_adj, x_weighted=eng.x_weighted, scale=eng.scale_factors, probe=probe, refused=refused,
                   reductions=eng.library_reductions))
    eng.dev.comm_destroy()


def test_collective_inside_the_library_at_200_samples():
    """dn_init_allreduce / dn_outer_allreduce on 3 * 200 + 4 = 604 doubles and dn_comm_allreduce at its cap of 772 (one past it is
    refused), at the one world size a single GPU offers, against the same run without the library's collective."""
    import torch.multiprocessing as mp
    from degnorm_amd.nmf_mpi import ShardedNMFOA, LocalComm
    ctx = mp.get_context('spawn')
    out_q = ctx.Queue()
    proc = ctx.Process(target=_libcomm_worker_200, args=(out_q,))
    proc.start()
    res = out_q.get(timeout=120)
    proc.join(timeout=60)
    assert proc.exitcode == 0
    np.testing.assert_array_equal(res['probe'], np.arange(772, dtype=np.float64))
    assert res['refused'] and res['reductions'] == 1 + 2
    p, covs, reads = _cohort_200()
    eng = ShardedNMFOA(comm=LocalComm(), device=0, degnorm_iter=2, nmf_iter=3)
    eng.load(covs, reads)
    eng.run(want_estimates=False)
    np.testing.assert_allclose(res['rho'], eng.rho, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(res['x_adj'], eng.x_adj, rtol=1e-12)
    np.testing.assert_allclose(res['x_weighted'], eng.x_weighted, rtol=1e-12)
    np.testing.assert_allclose(res['scale'], eng.scale_factors, rtol=1e-12)


def test_unchanged_below_65_and_refused_above_256():
    from degnorm_amd import _lib
    lib = _lib.load()
    assert lib.dn_p_supported(65) == 0 and lib.dn_p_supported(64) == 1
    assert _lib.p_max() == 256
    dev = _lib.Device(0)
    try:
        dev.upload([synth.synth_gene(3, g, 64, 100, 300)[0] for g in range(4)])
        assert dev.class_kernel_name(0) == 'k_baseline<64,256>'                 # the templated family ends at 64
        dev.upload([synth.synth_gene(3, g, 10, 6000, 9000)[0] for g in range(4)])      # longer than the narrow class takes
        assert dev.class_kernel_name(0) == 'k_baseline<10,256>'
        with pytest.raises(_lib.DegnormAmdError) as err:
            dev.upload([np.ones((257, 50))])
        assert '({0})'.format(_lib.DN_E_UNSUPPORTED) in str(err.value) or 'error {0}'.format(_lib.DN_E_UNSUPPORTED) in str(err.value)
        assert '256' in str(err.value)
    finally:
        dev.close()
