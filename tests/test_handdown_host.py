"""
Hand-down of a gene to the next narrower class (csrc/dn_kernels.hpp k_baseline, csrc/dn_api.hip dn_baseline_iteration): which nmf()
call of a gene is the first that the donor class does NOT make, restated in Python from n0, bins, the dropped-bin sequence and the
class's threshold, and checked against the CPU oracle's traces.  tests/test_gpu_handdown.py imports the restatement to predict how
many genes each class parks.
"""
import numpy as np

from degnorm_amd import synth


def call_widths(n0, bins, drops):
    """Active columns of every nmf() call of a gene's drop loop: call 0 runs on the n0 high-coverage columns, call k after k bins
    have been dropped.  split_into_chunks (utils.py:176-192): bins of ceil(n0 / bins) columns, the last one shorter; `drops` are
    indexes into the CURRENT bin list (trace[8:], nmf.py:291)."""
    csize = -(-int(n0) // int(bins))
    n_bins = -(-int(n0) // csize)
    lens = [min(csize, int(n0) - b * csize) for b in range(n_bins)]
    widths = [int(n0)]
    for d in drops:
        lens.pop(int(d))
        widths.append(sum(lens))
    return widths


def park_call(n0, bins, drops, n_calls, threshold):
    """Index k >= 1 of the call before which a class with `threshold` parks the gene: the first drop-loop call the gene makes at no
    more than `threshold` columns.  None: the gene is never parked (it leaves after the first call, or never gets that narrow)."""
    if threshold <= 0:
        return None
    widths = call_widths(n0, bins, drops)
    for k in range(1, min(int(n_calls), len(widths))):
        if widths[k] <= threshold:
            return k
    return None


def gene_class(length, split_len, tiny_len):
    return 0 if length > split_len else (1 if length > tiny_len else 2)


def predicted_parked(lengths, traces, bins, split_len, tiny_len, thresholds):
    """Genes each class parks (one count per class) in one iteration whose counters are `traces` (n x TRACE_LEN, the oracle's or the
    device's): class c hands down to c + 1 only if that class has genes of its own, and the pair class to nobody."""
    cls = [gene_class(L, split_len, tiny_len) for L in lengths]
    out = [0, 0, 0]
    for c in (0, 1):
        if (c + 1) not in cls:
            continue
        for L, tr, cg in zip(lengths, traces, cls):
            if cg == c and park_call(tr[0], bins, tr[8:8 + min(int(tr[5]), 32)], tr[1], thresholds[c]) is not None:
                out[c] += 1
    return out


def handdown_genes(p=10):
    """The genes of the hand-down tests: lengths on either side of the class boundaries 600 and 300 (DN_SPLIT_LEN / DN_TINY_LEN), for
    each length a few draws so that some run the drop loop to its end and some leave after one call."""
    covs = []
    for k, L in enumerate((301, 320, 599, 600, 601, 640, 900, 250, 300)):
        for g in range(4):
            covs.append(synth.synth_gene(61, 16 * k + g, p, L, L)[0])
        covs.append(synth.pileup_gene(62, 16 * k, p, L, L)[0])
    return covs


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
