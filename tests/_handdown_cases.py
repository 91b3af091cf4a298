"""
Shared cases of the hand-down tests (tests/test_handdown_host.py on the CPU, tests/test_gpu_handdown.py on the device): the
restatement of which nmf() call a donor class does not make, the gene sets, the sample counts, the parameter sets and one cached
oracle run per (gene set, sample count, parameter set).  Test infrastructure only; nothing here touches a GPU.
"""
import os
import sys
import time
import zlib

import numpy as np

from degnorm_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import fuzz_parity                                             # noqa: E402

# the class boundaries and the hand-down widths the tests set through the environment (read at the upload)
SPLIT, TINY, COLS = 600, 300, (400, 200)
ENV = {'DN_SPLIT_LEN': str(SPLIT), 'DN_TINY_LEN': str(TINY), 'DN_HANDDOWN_COLS': '%d,%d' % COLS}

P_THREE_CLASSES = (2, 3, 6, 9, 12)      # wide, narrow and pair class; 2 / 3 / 6 / 9 / 12 cover each register-tier width of rt_cols
P_TWO_CLASSES = (13, 16, 17, 24)        # no pair class and no register tier (hand_cols = the LDS columns); 17 and 24: the row solver
P_ALL = P_THREE_CLASSES + (10,) + P_TWO_CLASSES
# (bins, T, min_high_coverage): the shipped values; few and many bins (32 = HAND_MAX_BINS, the record full); few inner iterations
PARAM_SETS = ((20, 12, 50), (5, 12, 50), (32, 12, 50), (20, 3, 50), (32, 1, 10))
X_LENGTHS = (320, 599, 601, 900)        # the fuzz generators' lengths: a narrow gene, either side of DN_SPLIT_LEN, a wide gene
X_DRAWS = 3
X_PARAMS = PARAM_SETS[0]                # the parameter set of the x16 = 0 and the decay / holes runs
P_X16 = (2, 6, 10, 12, 16, 24)          # their sample counts
OTHER_KINDS = (('decay', 10), ('decay', 16), ('holes', 10), ('holes', 13))
SEED = 1
EXIT_REFINED, EXIT_REFINE_FALLBACK, EXIT_NOT_FOUND_FALLBACK = 4, 5, 6
LOOP_NATURAL, LOOP_PERFECT, LOOP_VALUE_ERROR, LOOP_ZERO_ROWSUM, LOOP_MIN_BINS = 0, 1, 2, 3, 4


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


def parked_genes(lengths, traces, bins, split_len, tiny_len, thresholds):
    """Per class, the genes it parks in one iteration whose counters are `traces` (n x TRACE_LEN, the oracle's or the device's):
    class c hands down to c + 1 only if that class has genes of its own, and the pair class to nobody."""
    cls = [gene_class(L, split_len, tiny_len) for L in lengths]
    out = [[], [], []]
    for c in (0, 1):
        if (c + 1) not in cls:
            continue
        for g, (tr, cg) in enumerate(zip(traces, cls)):
            if cg == c and park_call(tr[0], bins, tr[8:8 + min(int(tr[5]), 32)], tr[1], thresholds[c]) is not None:
                out[c].append(g)
    return out


def predicted_parked(lengths, traces, bins, split_len, tiny_len, thresholds):
    """How many genes each class parks (one count per class), see parked_genes."""
    return [len(v) for v in parked_genes(lengths, traces, bins, split_len, tiny_len, thresholds)]


def handdown_genes(p=10):
    """The genes of the hand-down tests: lengths on either side of the class boundaries 600 and 300 (DN_SPLIT_LEN / DN_TINY_LEN), for
    each length a few draws so that some run the drop loop to its end and some leave after one call."""
    covs = []
    for k, L in enumerate((301, 320, 599, 600, 601, 640, 900, 250, 300)):
        for g in range(4):
            covs.append(synth.synth_gene(61, 16 * k + g, p, L, L)[0])
        covs.append(synth.pileup_gene(62, 16 * k, p, L, L)[0])
    return covs


def bin_means(oracle, cov, scale, pset, drops):
    """The bin means the drop loop chooses from (nmf.py:280-291) after the bins `drops` have gone, restated on the oracle's nmf():
    per column the largest squared relative residual of the over-approximation, averaged per surviving bin."""
    bins, T, _ = pset
    F = np.asarray(cov, dtype=np.float64) / np.asarray(scale, dtype=np.float64)[:, None]
    Fb = F[:, F.max(axis=0) > 0.1 * F.max()]                       # get_high_coverage_idx, nmf.py:66-76
    n0 = Fb.shape[1]
    csize = -(-n0 // bins)
    lens = [min(csize, n0 - b * csize) for b in range(-(-n0 // csize))]
    for step in range(len(drops) + 1):
        K, E = oracle.nmf(Fb, T)
        KE = K * E
        if step > 0:
            KE = np.maximum(KE, Fb)                                # nmf.py:318
        res = (((KE - Fb) / (Fb + 1.0)) ** 2).max(axis=0)
        edges = np.concatenate(([0], np.cumsum(lens)))
        means = [float(res[edges[b]:edges[b + 1]].sum() / lens[b]) for b in range(len(lens))]
        if step == len(drops):
            return means
        d = int(drops[step])
        Fb = np.delete(Fb, np.arange(edges[d], edges[d + 1]), axis=1)
        lens.pop(d)


TIE_RTOL = 1e-12        # two bin means closer than this are the same number added in another order (tens of addends of ~1e-16 each)


def first_tie_flip(oracle, cov, scale, pset, drops_dev, drops_ora):
    """Where two dropped-bin sequences part: None if they are equal; otherwise (k, relative gap of the two bins' means at drop k in the
    oracle's own arithmetic).  A gap within TIE_RTOL is an exact tie between bins of equal content -- piecewise-constant coverage
    (synth.pileup_gene) has them -- which the summation order decides, on the device as in the reference."""
    drops_dev, drops_ora = [int(d) for d in drops_dev], [int(d) for d in drops_ora]
    if drops_dev == drops_ora:
        return None
    m = min(len(drops_dev), len(drops_ora))
    k = next((i for i in range(m) if drops_dev[i] != drops_ora[i]), m)
    if k == m:
        return k, float('inf')                                     # one sequence is a prefix of the other: no tie explains that
    means = bin_means(oracle, cov, scale, pset, drops_ora[:k])
    a, b = means[drops_dev[k]], means[drops_ora[k]]
    return k, abs(a - b) / max(abs(b), 1e-300)


def tiny_len(p):
    """The pair-class boundary the device uses under ENV: cohorts of 13 samples and more have no pair class."""
    return TINY if p <= 12 else 0


def donor_classes(p):
    return (0, 1) if p <= 12 else (0,)


def scales(p):
    return np.linspace(0.9, 1.2, p)


def is_x16(cov):
    """What k_row_max finds: every count is a whole number of at most 65535 (the register tier may carry the counts packed)."""
    return bool(np.all(cov == np.floor(cov)) and cov.max() <= 65535.0)


_GENES = {}


def genes(kind, p):
    """The gene set `kind` for p samples, built once: 'base' = handdown_genes(p); 'deep' = the same times 256 (most genes hold
    counts beyond 16 bits, every value still exact in fp32, the branch structure close to the original's); 'fractional', 'decay'
    and 'holes' = the generators of that name in tools/fuzz_parity.py at X_LENGTHS, X_DRAWS draws each (the `steps` generator is
    left out: its ties are decided by summation order)."""
    key = (kind, p)
    if key not in _GENES:
        if kind == 'base':
            covs = handdown_genes(p)
        elif kind == 'deep':
            base = genes('base', p)
            covs = [c * 256.0 for c in base]
            # the shallow genes of the donor classes stay below 65536 at that factor (at p = 2 all wide genes but one): once more, deeper
            covs += [c * 4096.0 for c in base if c.shape[1] in X_LENGTHS and c.max() * 256.0 <= 65535.0]
            assert max(float(c.max()) for c in covs) < 2.0 ** 24
        else:
            rng = np.random.default_rng([SEED, zlib.crc32(kind.encode()), p])
            covs = [fuzz_parity.make_gene(rng, p, L, kind) for L in X_LENGTHS for _ in range(X_DRAWS)]
            # none of these is short enough for the pair class: the base set's pair genes go with them, so that the narrow class
            # has somebody to hand to
            covs += [c for c in genes('base', p) if c.shape[1] <= TINY]
        _GENES[key] = covs
    return _GENES[key]


_ORACLE = {}
ORACLE_SECONDS = {}                     # what each oracle batch took, by the key of oracle_run


def oracle_run(oracle, kind, p, pset, scale=None):
    """(rho, flags, trace) of the oracle on genes(kind, p) with the parameter set (bins, T, min_high_coverage), computed once and
    shared between the tests; callers leave the arrays unchanged."""
    key = (kind, p, pset, None if scale is None else tuple(scale))
    if key not in _ORACLE:
        bins, T, mhc = pset
        covs = genes(kind, p)
        t0 = time.perf_counter()
        res = oracle.baseline_batch(covs, scales(p) if scale is None else scale,
                                    oracle.make_params(nmf_iter=T, bins=bins, min_high_coverage=mhc))
        ORACLE_SECONDS[key] = time.perf_counter() - t0
        for a in res[:3]:
            a.setflags(write=False)
        _ORACLE[key] = res[:3]
    return _ORACLE[key]


def parked_of(oracle, kind, p, pset, thresholds=COLS):
    """Per class, the genes of genes(kind, p) that the device is to park under ENV, from the oracle's traces."""
    lengths = [c.shape[1] for c in genes(kind, p)]
    return parked_genes(lengths, oracle_run(oracle, kind, p, pset)[2], pset[0], SPLIT, tiny_len(p), thresholds)


def equality_case(oracle, p=10, pset=PARAM_SETS[0]):
    """A wide-class gene of the base set with at least two calls and the width w of its last call: with the wide threshold w the gene
    parks before that call, with w - 1 never (widths fall strictly).  The gene with the widest such call is taken, and the narrow
    genes go with it so that the wide class has somebody to hand to.  Returns (gene indexes, index of the wide gene in them, w)."""
    covs = genes('base', p)
    trace = oracle_run(oracle, 'base', p, pset)[2]
    best = None
    for g, (c, tr) in enumerate(zip(covs, trace)):
        if c.shape[1] > SPLIT and tr[1] >= 2:
            w = call_widths(tr[0], pset[0], tr[8:8 + tr[5]])[tr[1] - 1]
            if best is None or w > best[1]:
                best = (g, w)
    assert best is not None
    narrow = [g for g, c in enumerate(covs) if tiny_len(p) < c.shape[1] <= SPLIT]
    return [best[0]] + narrow, 0, best[1]
