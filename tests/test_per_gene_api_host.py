"""
The reference's per-gene methods of GeneNMFOA (degnorm/nmf.py:55-453) and the module functions of degnorm/nmf_mpi.py
(:10-445), host side: the C symbols of the float64 path, the signatures, the host-only bookkeeping (shift_bins,
get_high_coverage_idx, the systematic sample) and the absence of a CPU fallback.  No GPU needed.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's signatures (degnorm/nmf.py, degnorm/nmf_mpi.py v0.1.4), self omitted
CLASS_METHODS = {
    'rank_one_approx': ('(x)', True),
    'get_high_coverage_idx': ('(x)', True),
    'nmf': ('(x, factors=False)', False),
    'ratio_svd': ('(x)', False),
    'run_ratio_svd_serial': ('(x)', False),
    'adjust_coverage_curves': ('(dat)', False),
    'shift_bins': ('(bins, dropped_bin)', True),
    'baseline_selection': ('(F)', False),
    'run_baseline_selection_serial': ('(x)', False),
    'par_apply_baseline_selection': ('(dat, degnorm_iter)', False),
    '_systematic_sample': ('(n, take_every)', True),
    'downsample_2d': ('(x, by_row=True)', False),
}
MODULE_FUNCTIONS = {
    'rank_one_approx': '(x)',
    'get_high_coverage_idx': '(x)',
    'nmf': '(x, factors=False, nmf_iter=100)',
    'ratio_svd': '(x)',
    'run_ratio_svd_serial': '(x)',
    'shift_bins': '(bins, dropped_bin)',
    'adjust_coverage_curves': '(dat, scale_factors)',
    'correct_di_scores': '(rho, x_weighted, x_adj)',
    'systematic_sample': '(n, take_every=1)',
    'downsample_2d': '(x, downsample_rate=1, by_row=True)',
    'baseline_selection': '(F, nmf_iter=100, downsample_rate=1, min_high_coverage=20, bins=20, bin_frac=0.2, '
                          'skip_baseline_selection=False)',
    'run_baseline_selection_serial': '(x, **kwargs)',
}


def test_float64_path_symbols_are_exported():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    from degnorm_amd import _lib, build
    build.build_library()
    syms = ge.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ('dn_nmf_f64', 'dn_baseline_selection_f64', 'dn_last_f64_ms'):
        assert s in syms, s + ' is not declared in include/degnorm_amd.h'
        assert hasattr(lib, s), 'missing C ABI symbol ' + s
    _lib.load()                                                     # the ctypes prototypes of the new entry points load


def test_class_methods_have_the_reference_signatures():
    from degnorm_amd.nmf import GeneNMFOA
    for name, (sig, static) in CLASS_METHODS.items():
        assert hasattr(GeneNMFOA, name), name
        raw = inspect.getattr_static(GeneNMFOA, name)
        assert isinstance(raw, staticmethod) == static, name
        fn = getattr(GeneNMFOA, name)
        got = str(inspect.signature(fn))
        if not static:
            got = str(inspect.signature(getattr(GeneNMFOA(), name)))
        assert got == sig, (name, got, sig)


def test_module_functions_have_the_reference_signatures():
    from degnorm_amd import nmf_mpi
    for name, sig in MODULE_FUNCTIONS.items():
        assert name in nmf_mpi.__all__, name
        assert str(inspect.signature(getattr(nmf_mpi, name))) == sig, name


def test_shift_bins_reproduces_the_reference_bounds():
    """kat.npz shift_bounds0..2: split_into_chunks(range(41), 5), then bins 1, 0, 2 dropped one after the other."""
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd import nmf_mpi
    from degnorm_amd.utils import split_into_chunks
    K = golden('kat')
    for shift in (GeneNMFOA.shift_bins, nmf_mpi.shift_bins):
        bins = split_into_chunks(list(range(41)), 5)
        for d, key in zip([1, 0, 2], ['shift_bounds0', 'shift_bounds1', 'shift_bounds2']):
            del bins[d]
            bins = shift(bins, dropped_bin=d)
            flat = [k for b in bins for k in b]
            assert flat == list(range(len(flat)))                   # consecutive from 0
            np.testing.assert_array_equal([b[0] for b in bins] + [bins[-1][-1] + 1], K[key])
    assert GeneNMFOA.shift_bins([[0, 1], [2, 3]], 2) == [[0, 1], [2, 3]]      # dropped the last bin: unchanged
    assert GeneNMFOA.shift_bins([[4, 5]], 0) == [[4, 5]]                      # one bin left: unchanged


def test_get_high_coverage_idx():
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd import nmf_mpi
    x = np.array([[0., 1., 10., 0.5, 1.0000001],
                  [0., 0., 2., 1.0, 0.]])
    for f in (GeneNMFOA.get_high_coverage_idx, nmf_mpi.get_high_coverage_idx):
        np.testing.assert_array_equal(f(x), [2, 4])                # strictly above 0.1 * max
    rng = np.random.RandomState(3)
    y = rng.lognormal(size=(5, 300))
    np.testing.assert_array_equal(GeneNMFOA.get_high_coverage_idx(y), np.flatnonzero(y.max(axis=0) > 0.1 * y.max()))


def test_systematic_sample_and_downsample_2d_follow_the_reference():
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd import nmf_mpi
    x = np.arange(3 * 50, dtype=float).reshape(3, 50)
    for seed in (0, 7, 123):
        np.random.seed(seed)
        start = np.random.choice(7)                                 # the reference's draw (nmf.py:422)
        np.random.seed(seed)
        idx = GeneNMFOA._systematic_sample(50, 7)
        np.testing.assert_array_equal(idx, np.arange(start, 50, 7))
        np.random.seed(seed)
        xs, idx2 = GeneNMFOA(downsample_rate=7).downsample_2d(x, by_row=False)
        np.testing.assert_array_equal(idx2, np.arange(start, 50, 7))
        np.testing.assert_array_equal(xs, x[:, start::7])
        np.random.seed(seed)
        xr, idx3 = nmf_mpi.downsample_2d(x.T, downsample_rate=7, by_row=True)
        np.testing.assert_array_equal(xr, x.T[start::7, :])
        np.random.seed(seed)
        np.testing.assert_array_equal(nmf_mpi.systematic_sample(50, 7), np.arange(start, 50, 7))
    np.random.seed(5)
    one = np.random.choice(4)
    np.random.seed(5)
    assert GeneNMFOA._systematic_sample(4, 9) == one                # take_every >= n: a single index
    same, all_idx = GeneNMFOA().downsample_2d(x)                     # rate 1: nothing drawn, everything kept
    assert same is x and np.array_equal(all_idx, np.arange(3))
    with pytest.raises(ValueError):
        GeneNMFOA(downsample_rate=50).downsample_2d(x, by_row=False)     # rate >= gene length
    with pytest.raises(ValueError):
        nmf_mpi.downsample_2d(x, downsample_rate=60, by_row=False)


def test_host_helpers_of_the_module():
    from degnorm_amd import nmf_mpi
    from degnorm_amd.nmf import GeneNMFOA
    dat = [np.arange(6, dtype=float).reshape(2, 3), np.ones((2, 4))]
    s = np.array([2.0, 4.0])
    for a, F in zip(nmf_mpi.adjust_coverage_curves(dat, s), dat):
        np.testing.assert_array_equal(a, F / s[:, None])
    m = GeneNMFOA()
    m.scale_factors = s
    for a, F in zip(m.adjust_coverage_curves(dat), dat):
        np.testing.assert_array_equal(a, F / s[:, None])
    rho = np.array([[0.1, 0.2], [0.0, 0.0]])
    xw, xa = np.array([[1., 2.], [3., 4.]]), np.array([[2., 4.], [4., 5.]])
    out = nmf_mpi.correct_di_scores(rho, xw, xa)
    np.testing.assert_array_equal(out[1], 1 - xw.sum(axis=0) / xa.sum(axis=0))
    np.testing.assert_array_equal(out[0], [0.1, 0.2])


def test_shape_and_parameter_errors_come_before_the_device():
    """min(shape) < 2 is svds' ValueError; a bin_frac the device path does not implement is rejected, never ignored."""
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd import nmf_mpi
    for bad in (np.ones((1, 10)), np.ones((10, 1)), np.ones(10)):
        with pytest.raises(ValueError):
            GeneNMFOA().nmf(bad)
        with pytest.raises(ValueError):
            nmf_mpi.ratio_svd(bad)
        with pytest.raises(ValueError):
            GeneNMFOA.rank_one_approx(bad)
    with pytest.raises(ValueError, match='bin_frac'):
        nmf_mpi.baseline_selection(np.ones((3, 300)), bin_frac=0.3)


def test_per_gene_methods_fail_loudly_without_gpu():
    """No CPU fallback: without a HIP device the per-gene methods raise DegnormAmdError."""
    from degnorm_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a GPU is visible here')
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd import nmf_mpi
    x = np.random.RandomState(0).lognormal(size=(4, 30))
    with pytest.raises(_lib.DegnormAmdError):
        GeneNMFOA().nmf(x)
    with pytest.raises(_lib.DegnormAmdError):
        GeneNMFOA().baseline_selection(x)
    with pytest.raises(_lib.DegnormAmdError):
        GeneNMFOA.rank_one_approx(x)
    with pytest.raises(_lib.DegnormAmdError):
        nmf_mpi.nmf(x)
