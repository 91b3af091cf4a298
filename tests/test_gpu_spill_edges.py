"""
Device against the CPU oracle on genes that straddle every tier edge of the NMF pass (csrc/dn_kernels.hpp: register tier, LDS
tier, spill tier) in every gene class, with the criteria of test_gpu_parity.py: branch trace[:7] and flags exact, DI within
1e-9 relative.  The class boundaries and the on-chip capacity of a class come from the library (dn_class_lengths,
dn_class_tier_cols), not from literals, so the genes follow the tiers when a build moves them.
"""
import numpy as np
import pytest

from degnorm_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-11
T = 14            # inner iterations: the pass walks forwards on even and backwards on odd ones


def _flat(rng, p, n, L=0):
    """Flat, deep coverage over n bases: every one of them is an active column, so the gene's active width is exactly n.  L > n:
    padded with uncovered bases (never active) up to the length that puts the gene into the class wanted."""
    cov = rng.poisson(np.outer(rng.uniform(150., 400., p), np.ones(n))).astype(float)
    return cov if L <= n else np.hstack([cov, np.zeros((p, L - n))])


def _class_of(L, split, tiny):
    return 0 if L > split else (2 if L <= tiny else 1)                  # split = 0: one class, class 0


# p = 10: the benchmark's cohort (register tier, raw-unit pass); 9, 11: odd p (the padded half of the last spill plane); 16: no
# register tier, and the later read-only sweeps of the Gram matrix run over the spill state; 25: the wide-cohort path (Gram
# matrix on the matrix cores, mg_core), odd as well
@pytest.mark.parametrize('p', [10, 9, 11, 16, 25])
def test_genes_on_every_tier_edge_agree_with_the_oracle(oracle, p):
    from degnorm_amd import _lib
    rng = np.random.default_rng(9000 + p)
    dev = _lib.Device(0)
    try:
        split, tiny = dev.class_lengths(p)
        # the longest gene of each class sizes the class's scratch slot and shows its on-chip capacity (split = 0: one class)
        longest = {0: 2 * split, 1: split} if split > 0 else {0: 4000}
        if tiny > 0:
            longest[2] = tiny
        floor = {0: split + 1, 1: tiny + 1, 2: 1}                          # the shortest gene of each class
        probe = [_flat(rng, p, L) for L in longest.values()]
        dev.upload(probe)
        dev.baseline_iteration(np.ones(p), nmf_iter=2)
        cap = {}
        for cls in longest:
            reg, lds = dev.class_tier_cols(cls)
            assert lds > 0 and reg >= 0
            cap[cls] = reg + lds                                           # first column of the spill tier (counts within 16 bits)
        assert [_class_of(L, split, tiny) for L in longest.values()] == list(longest)
        covs, edge_of = list(probe), {}
        drop_candidates = {}
        for cls, kS0 in cap.items():
            assert kS0 + 65 < longest[cls], 'class %d keeps its longest gene on chip: no spill tier to test' % cls
            for d in (-1, 0, 1, 63, 64, 65):
                L = max(kS0 + d, floor[cls])
                assert _class_of(L, split, tiny) == cls
                edge_of[len(covs)] = (cls, d)
                covs.append(_flat(rng, p, kS0 + d, L))
            big = _flat(rng, p, kS0 + 65, floor[cls])
            big[0, :7] = 70000.0                                           # not packable into 16 bits: the body that re-reads its counts
            covs.append(big)
            # degraded genes a little beyond the on-chip capacity: the drop loop shrinks them back below it
            lo = max(kS0 + 40, floor[cls])
            hi = min(lo + 360, longest[cls])
            drop_candidates[cls] = list(range(len(covs), len(covs) + 6))
            for g in range(6):
                covs.append(synth.synth_gene(77 + p, 100 * cls + g, p, lo, hi)[0])
        scale = np.linspace(0.85, 1.25, p)
        dev.upload(covs)
        rho, flags, trace = dev.baseline_iteration(scale, nmf_iter=T)
        for cls in longest:                                                # the re-upload kept the capacity the genes were cut to
            assert sum(dev.class_tier_cols(cls)) == cap[cls]
    finally:
        dev.close()
    rho_o, flags_o, trace_o, _ = oracle.baseline_batch(covs, scale, oracle.make_params(nmf_iter=T))
    for i, (cls, d) in edge_of.items():                                    # the edge genes really have the active width they were cut to
        assert trace_o[i, 0] == cap[cls] + d and trace_o[i, 1] >= 1
    np.testing.assert_array_equal(trace[:, :7], trace_o[:, :7])
    np.testing.assert_array_equal(flags, flags_o)
    np.testing.assert_allclose(rho, rho_o, rtol=RTOL, atol=ATOL)
    # at least one gene starts in the spill tier and is shrunk back on chip by the drop loop: its later calls average at most the
    # on-chip capacity, so at least one of them fits (trace: 0 = initial active columns, 1 = nmf() calls, 2 = sum of their columns)
    back_on_chip = 0
    for cls, ids in drop_candidates.items():
        for i in ids:
            n0, calls, cols = int(trace[i, 0]), int(trace[i, 1]), int(trace[i, 2])
            if n0 > cap[cls] and calls >= 2 and (cols - n0) / (calls - 1) <= cap[cls]:
                back_on_chip += 1
    assert back_on_chip >= 1
