"""
The reference's per-gene NMF-OA helpers -- GeneNMFOA.rank_one_approx ... downsample_2d (degnorm/nmf.py:55-453) and the
module-level functions of degnorm/nmf_mpi.py (:10-445) -- on the float64-input device path.

The factorisations run in HIP kernels (dn_nmf_f64, dn_baseline_selection_f64 in include/degnorm_amd.h): one launch per
call, on float64 inputs as given, in buffers of their own (a handle's resident coverage and outer-iteration state are never
touched).  The index bookkeeping (get_high_coverage_idx, shift_bins, the systematic sample) is host numpy, as in the
reference.  There is no CPU fallback: without the HIP library or a GPU every device call raises DegnormAmdError.

nmf.py (class methods) and nmf_mpi.py (free functions) are thin wrappers over this module.  The device calls take a
zero-argument `get_dev` returning the Device to use, so that inputs are checked (ValueError) before a device is opened.
"""
import os

import numpy as np

from . import _lib

_static_dev = None


def static_device():
    """One Device per process for callers without a GeneNMFOA instance (static methods, nmf_mpi functions): LOCAL_RANK or 0."""
    global _static_dev
    if _static_dev is None:
        _static_dev = _lib.Device(int(os.environ.get('LOCAL_RANK', 0)))
    return _static_dev


def as_matrix(x):
    """float64 2-d array with at least 2 rows and 2 columns (svds(k=1) raises ValueError otherwise, nmf.py:63)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('expected a 2-d array, got {0} dimension(s)'.format(x.ndim))
    if min(x.shape) < 2:
        raise ValueError('k must be between 1 and min(A.shape) - 1: matrix of shape {0}'.format(x.shape))
    return x


def check_status(status, what):
    """Raise DegnormAmdError naming the first non-zero per-matrix device status."""
    bad = np.flatnonzero(np.asarray(status) != 0)
    if bad.size:
        k = int(bad[0])
        s = int(status[k])
        raise _lib.DegnormAmdError('{0}: matrix {1} of {2}: device status {3} ({4}){5}'.format(
            what, k, len(status), s, _lib.STATUS_NAMES.get(s, 'unknown'),
            '' if bad.size == 1 else '; {0} matrices failed'.format(bad.size)))


# -- host index bookkeeping -------------------------------------------------------------------------------------------
def get_high_coverage_idx(x):
    """Positions whose sample-wise maximum exceeds 10 % of the matrix maximum (nmf.py:66-76)."""
    x = np.asarray(x)
    return np.where(x.max(axis=0) > 0.1 * x.max())[0]


def shift_bins(bins, dropped_bin):
    """
    Renumber the bins after position `dropped_bin` was deleted from `bins` so that they stay consecutive from where the
    previous bin ends (nmf.py:160-187); `bins` (a list of lists of int) is updated in place and returned.
    """
    if dropped_bin == len(bins) or len(bins) == 1:
        return bins
    if dropped_bin == 0:
        gap = bins[0][0]
    else:
        gap = bins[dropped_bin][0] - bins[dropped_bin - 1][-1] - 1
    for b in range(dropped_bin, len(bins)):
        bins[b] = [k - gap for k in bins[b]]
    return bins


def systematic_sample(n, take_every=1):
    """
    Every take_every-th index of range(n) from a random start below take_every, drawn from the global np.random stream
    (nmf.py:408-425); take_every >= n draws a single index.
    """
    if take_every >= n:
        return int(np.random.choice(n))
    start = np.random.choice(take_every)
    return np.arange(start, n, step=take_every, dtype=int)


def downsample_2d(x, downsample_rate=1, by_row=True):
    """Systematic sample of the rows (or columns) of x: (sampled x, indices) (nmf.py:427-453)."""
    Li = x.shape[0 if by_row else 1]
    if downsample_rate == 1:
        return x, np.arange(0, Li)
    if downsample_rate >= Li:
        raise ValueError('Cannot downsample at a rate < 1 / length(gene)')
    idx = systematic_sample(Li, take_every=downsample_rate)
    return (x[idx, :], idx) if by_row else (x[:, idx], idx)


def adjust_coverage_curves(dat, scale_factors):
    """F / s_i row by row (nmf.py:142-146)."""
    return [(F.T / scale_factors).T for F in dat]


def correct_di_scores(rho, x_weighted, x_adj):
    """Genes whose DI row is all zero get the sample-average DI score, in place (nmf.py:148-158); returns rho."""
    zero = rho.max(axis=1) == 0
    if np.sum(zero) > 0:
        rho[zero, :] = 1 - (x_weighted.sum(axis=0) / x_adj.sum(axis=0))
    return rho


# -- device calls -----------------------------------------------------------------------------------------------------
def _nmf_batch(get_dev, mats, mode, nmf_iter, want_est, what):
    mats = [as_matrix(x) for x in mats]
    if not mats:
        return [], [], []
    p = mats[0].shape[0]
    if any(x.shape[0] != p for x in mats):
        raise ValueError('{0}: all matrices of one batch need the same number of rows'.format(what))
    K, E, est, status = get_dev().nmf_f64(mats, mode, nmf_iter, want_est)
    check_status(status, what)
    return K, E, est


def rank_one_approx(get_dev, x):
    """(K p x 1, E 1 x n) with K E the best rank-one approximation of x (nmf.py:55-64)."""
    K, E, _ = _nmf_batch(get_dev, [x], _lib.NMF_RANK_ONE, 0, False, 'rank_one_approx')
    return K[0].reshape(-1, 1).copy(), E[0].reshape(1, -1).copy()


def nmf(get_dev, x, nmf_iter=100, factors=False):
    """NMF-OA of x with nmf_iter Lagrangian iterations (nmf.py:78-107): (K, E) or K.dot(E)."""
    K, E, est = _nmf_batch(get_dev, [x], _lib.NMF, abs(int(nmf_iter)), not factors, 'nmf')
    if factors:
        return K[0].reshape(-1, 1).copy(), E[0].reshape(1, -1).copy()
    return est[0].copy()


def ratio_svd_list(get_dev, mats):
    """max(K E, x) of every matrix, one device launch for the batch (nmf.py:109-124)."""
    mats = list(mats)
    if not mats:
        return []
    out = [None] * len(mats)
    rows = {}
    for k, x in enumerate(mats):                       # one launch per distinct row count (a batch shares p)
        rows.setdefault(np.shape(x)[0] if np.ndim(x) == 2 else -1, []).append(k)
    for _, ks in sorted(rows.items()):
        _, _, est = _nmf_batch(get_dev, [mats[k] for k in ks], _lib.NMF_RATIO, 0, True, 'ratio_svd')
        for k, e in zip(ks, est):
            out[k] = e.copy()
    return out


def baseline_selection_list(get_dev, mats, nmf_iter=100, bins=20, min_high_coverage=50, downsample_rate=1,
                            skip_baseline_selection=False, p=None):
    """
    baseline_selection (nmf.py:189-372) of every matrix in one device launch, float64 as given.  Returns a list of
    (rho (p,) unclipped, estimate (p x L), ran bool).  With downsample_rate > 1 the systematic-sample start of each gene is
    drawn here, in gene order, from np.random (nmf.py:222-224 -> :422).
    """
    mats = [np.asarray(F, dtype=np.float64) for F in mats]
    if not mats:
        return []
    for F in mats:
        if F.ndim != 2:
            raise ValueError('Not all coverage matrices are 2-d arrays!')
    q = mats[0].shape[0] if p is None else int(p)
    if any(F.shape[0] != q for F in mats):
        raise ValueError('coverage matrices must have p = {0} rows'.format(q))
    if q < 2:
        raise ValueError('k must be between 1 and min(A.shape) - 1: {0} sample(s)'.format(q))
    rate = abs(int(downsample_rate))
    ds = None
    if rate > 1:
        ds = np.zeros(len(mats), dtype=np.int64)
        for k, F in enumerate(mats):
            if rate >= F.shape[1]:
                raise ValueError('Cannot downsample at a rate < 1 / length(gene)')
            ds[k] = np.random.choice(rate)             # systematic_sample's start draw (nmf.py:422)
    rho, flags, trace, est = get_dev().baseline_selection_f64(mats, nmf_iter=nmf_iter, bins=bins, min_high_coverage=min_high_coverage,
                                                        downsample_rate=rate, skip_baseline_selection=skip_baseline_selection,
                                                        ds_start=ds, want_est=True)
    check_status(trace[:, 6], 'baseline_selection')
    return [(rho[k].copy(), est[k].copy(), bool(flags[k])) for k in range(len(mats))]
