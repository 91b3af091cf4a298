"""
The outer DegNorm update and the initial normalisation restated in numpy float64, as references for the O(n p) kernels of
csrc/dn_outer.hip (k_scale_reads and the family k_outer_partials, k_outer_reduce, k_outer_apply, k_init_partials <WR>, whose
two instantiations -- one sample per lane for at most 64 samples, four for 65 to 256 -- share everything below).

Reference lines (degnorm/nmf.py of the reference): the DI clip :398-399, the ran_baseline_selection column :403,
correct_di_scores :148-158, x_adj :575 and :581, the normalisation :584-587, the initial pass :524-533 -- in the formulation
of degnorm_amd/nmf_mpi.py (iterate, _reduce_and_update) and oracle.run: per-sample sums over the touched and the untouched
genes instead of the n x p matrices.

Every elementwise result is one or two IEEE double operations, formed here exactly as numpy forms them.  The sums come
twice: `*_partials` adds the terms with math.fsum (the correctly rounded sum: what any order of additions approximates),
`*_partials_ordered` adds them in the order the device documents, which is part of the kernels' results:

    wave w of block b adds genes 4 b + w + k * 4 * blocks (k = 0, 1, ...) in turn, starting from +0.0
    a block adds its four waves left to right: ((w0 + w1) + w2) + w3
    block b goes to running sum b % 8, blocks in increasing order
    the eight sums are combined as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))
    blocks = min(512, ceil(n / 4))

The partial vector is the device's: [A (p), B (p), W (p), four counts], 3 p + 4 doubles (include/degnorm_amd.h).
"""
import math

import numpy as np

ST_NO_CONVERGENCE = -4
MAX_BLOCKS = 512


def clip(rho_raw):
    """nmf.py:398-399.  (-0.0 is not < 0 and stays -0.0.)"""
    rho = np.array(rho_raw, dtype=np.float64)
    rho[rho > 0.9] = 0.9
    rho[rho < 0.] = 0.
    return rho


def untouched(rho_c):
    """nmf.py:155: genes that baseline selection left without a DI score."""
    return rho_c.max(axis=1) == 0


def outer_terms(rho_c, xw, status, flags):
    """The n x (3p + 4) terms whose column sums are the partial vector of an outer update."""
    u = untouched(rho_c)[:, None]
    with np.errstate(divide='ignore'):
        adj = xw / (1 - rho_c)                                        # nmf.py:575
    status, flags = np.asarray(status), np.asarray(flags)
    counts = np.stack([u[:, 0], status != 0, status == ST_NO_CONVERGENCE, flags != 0], axis=1).astype(np.float64)
    return np.concatenate([np.where(u, 0.0, adj), np.where(u, xw, 0.0), xw, counts], axis=1)


def init_rho(est_sums, cov_sums):
    return 1 - (cov_sums / (est_sums + 1))                            # nmf.py:526


def init_terms(est_sums, cov_sums, status, x):
    """The terms of the initial normalisation: A = read counts of the low genes, B = of all genes, W unused; #low, #failed."""
    low = init_rho(est_sums, cov_sums).max(axis=1) < 0.1              # nmf.py:529
    zero = np.zeros((len(x), 1))
    counts = np.concatenate([low[:, None].astype(np.float64), (np.asarray(status) != 0)[:, None].astype(np.float64), zero, zero], axis=1)
    return np.concatenate([np.where(low[:, None], x, 0.0), x, np.zeros_like(x), counts], axis=1)


def fsum_columns(terms):
    return np.array([math.fsum(col) for col in terms.T.tolist()])


def ordered_columns(terms):
    """The column sums of `terms` in the device's documented order (module docstring)."""
    n, m = terms.shape
    blocks = min(MAX_BLOCKS, (n + 3) // 4)
    nw = 4 * blocks
    acc = np.zeros((nw, m))
    for k in range(0, n, nw):                                         # every wave adds its next gene
        rows = terms[k:k + nw]
        acc[:len(rows)] = acc[:len(rows)] + rows
    acc = acc.reshape(blocks, 4, m)
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    a = np.zeros((8, m))
    for b in range(0, blocks, 8):                                     # block b to running sum b % 8
        rows = part[b:b + 8]
        a[:len(rows)] = a[:len(rows)] + rows
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def outer_partials(rho_c, xw, status, flags):
    return fsum_columns(outer_terms(rho_c, xw, status, flags))


def outer_partials_ordered(rho_c, xw, status, flags):
    return ordered_columns(outer_terms(rho_c, xw, status, flags))


def init_partials(est_sums, cov_sums, status, x):
    return fsum_columns(init_terms(est_sums, cov_sums, status, x))


def init_partials_ordered(est_sums, cov_sums, status, x):
    return ordered_columns(init_terms(est_sums, cov_sums, status, x))


def init_norm(partials, p):
    """nmf.py:530-531 from the partial vector of the initial pass: the low genes' sums when there is a low gene, else all."""
    count_sums = partials[:p] if partials[3 * p] > 0 else partials[p:2 * p]
    return count_sums / np.median(count_sums)


def scale_reads(x, norm):
    return x / norm                                                   # nmf.py:533


def derive(partials, p):
    """(avg_di or None, norm) from the partial vector of an outer update: nmf.py:157-158, :581-584 on per-sample sums."""
    A, B, W, n_untouched = partials[:p], partials[p:2 * p], partials[2 * p:3 * p], partials[3 * p]
    S = A + B                                                         # column sums of the first x_adj (nmf.py:575)
    avg_di = None
    if n_untouched > 0:
        avg_di = 1 - (W / S)                                          # nmf.py:157
        S = A + B / (1 - avg_di)                                      # column sums of the second x_adj (nmf.py:581)
    return avg_di, S / np.median(S)


def outer_apply(rho_c, xw, flags, ran, avg_di, norm, it):
    """correct_di_scores with the given average (None: nothing is replaced), x_adj, the next x_weighted, and column `it` of
    ran_baseline_selection (left alone when `it` is not a column of it).  Returns (rho, x_adj, x_weighted, ran)."""
    rho = np.array(rho_c, dtype=np.float64)
    if avg_di is not None:
        rho[untouched(rho_c), :] = avg_di                             # nmf.py:157
    with np.errstate(divide='ignore'):
        x_adj = xw / (1 - rho)                                        # nmf.py:581
    ran = np.array(ran, dtype=bool)
    if 0 <= it < ran.shape[1]:
        ran[:, it] = np.asarray(flags) != 0                           # nmf.py:403
    return rho, x_adj, xw / norm, ran                                 # nmf.py:587


def sum_bound(n, s_fsum):
    """|S - fsum| for n non-negative doubles added in ANY order: every partial sum is at most the total, each of the n - 1
    additions errs by at most 2^-53 of its result, and fsum itself by 2^-53 of the total: n * 2^-53 * total in all."""
    return n * 2.0 ** -53 * s_fsum
