"""
The partial register-tier body of the NMF pass (csrc/dn_kernels.hpp: a call with fewer columns than the register tier holds, n < RT * NT)
against the CPU oracle.  The body pads the gene's last round of the tier with zero columns and walks whole rounds unmasked, so the
widths that matter are those around a round's edge (NT - 1, NT, NT + 1, ...), the hand-over to the full body (RT * NT - 1, RT * NT), and
calls of the drop loop, where a narrower call finds the wider call's data in the registers it has to pad.  Every class (pair NT = 64,
narrow 128, wide 256) at p = 10 and at sample counts with another RT.
"""
import numpy as np
import pytest

from degnorm_amd import synth

pytestmark = pytest.mark.gpu

T = 20
MHC = 50
DROP_GENES = (1, 2, 6, 7, 16)             # synth.pileup_gene(31, g, p, 300, 2500): at least 3 nmf() calls for p = 2, 6, 10, 12 (checked below)


def _rt_cols(p):
    return min(12, 256 // (2 * p + (p + 1) // 2))                         # dn_kernels.hpp rt_cols<P, X16 = true>


def _gene(rng, p, L, m, scale):
    """A gene of length L whose first m columns are its high-coverage columns (get_high_coverage_idx on x / scale): the others stay just
    below 0.1 x max, and non-zero."""
    x = rng.poisson(np.outer(rng.uniform(150., 400., p), np.ones(L))).astype(float)
    top = (x[:, :m] / scale[:, None]).max()
    low = np.floor(0.099 * top * scale)[:, None] - rng.integers(0, 3, size=(p, L - m))
    assert low.min() >= 1.
    x[:, m:] = low
    return x


@pytest.mark.parametrize('p', [10, 2, 6, 12])
def test_partial_tier_widths_and_drop_loop_vs_oracle(device, oracle, p):
    split_len, tiny_len = device.class_lengths(p)
    rt = _rt_cols(p)
    assert tiny_len >= rt * 64 and split_len >= rt * 128 and tiny_len < split_len
    scale = np.linspace(0.85, 1.25, p)
    rng = np.random.default_rng(1600 + p)
    covs, want_n0 = [], []
    for nt, L in ((64, tiny_len), (128, split_len), (256, max(split_len + 1, rt * 256))):     # the length picks the class
        for m in (max(50, MHC), nt - 1, nt, nt + 1, 2 * nt, 3 * nt + 1, rt * nt - 1, rt * nt):
            assert m <= L
            covs.append(_gene(rng, p, L, m, scale))
            want_n0.append(m)
    n_width = len(covs)
    covs += [synth.pileup_gene(31, g, p, 300, 2500)[0] for g in DROP_GENES]
    assert len(covs) < 60
    rho_o, flags_o, trace_o, _ = oracle.baseline_batch(covs, scale, oracle.make_params(nmf_iter=T, min_high_coverage=MHC))
    np.testing.assert_array_equal(trace_o[:n_width, 0], want_n0)          # the genes have the widths they were built for
    assert (trace_o[n_width:, 1] >= 3).all()                              # a narrower call follows a wider one
    device.upload(covs)
    rho, flags, trace = device.baseline_iteration(scale, nmf_iter=T, min_high_coverage=MHC)
    assert device.split_length() == split_len and device.tiny_length() == tiny_len
    assert device.class_kernel_name(2) == 'k_baseline<{0},64>'.format(p)
    np.testing.assert_array_equal(trace[:, :7], trace_o[:, :7])
    np.testing.assert_array_equal(flags, flags_o)
    np.testing.assert_allclose(rho, rho_o, rtol=1e-8, atol=1e-10)
