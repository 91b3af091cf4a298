"""
The NMF C ABI (csrc/dn_api.hip) under the exit rule of dn_host.hpp, with all three gene classes -- and so all three streams of
the handle -- carrying a kernel: a call that is refused for its arguments or for the handle's state leaves the handle as it
was, and a handle that is uploaded to twice and then closed computes what fresh handles compute.  Argument and state
refusals only: the exits that a failing HIP call alone reaches are checked by reading the code.
"""
import ctypes

import numpy as np
import pytest

import _api_errors
from degnorm_amd import _lib, synth

pytestmark = pytest.mark.gpu

SEED = 14
LENGTHS_P4 = (200, 250, 300, 350, 450, 600, 650, 800, 900)      # DN_TINY_LEN = 300, DN_SPLIT_LEN = 600: three genes per class
LENGTHS_P10 = (300, 375, 450, 525, 600)


def _genes(p, lengths):
    return [synth.synth_gene(SEED, g, p, L, L)[0] for g, L in enumerate(lengths)]


def _scale(p):
    return np.linspace(0.8, 1.25, p)


def _run(dev):
    """Initial sums, one baseline iteration with estimates, the estimates: everything the three calls return."""
    est_sums, cov_sums, status = dev.ratio_svd_sums()
    rho, flags, trace = dev.baseline_iteration(_scale(dev.p), nmf_iter=5, want_estimates=True)
    return [est_sums, cov_sums, status, rho, flags, trace[:, :8].copy()] + [e.copy() for e in dev.fetch_estimates()]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.fixture
def three_classes(monkeypatch):
    monkeypatch.setenv('DN_SPLIT_LEN', '600')
    monkeypatch.setenv('DN_TINY_LEN', '300')


def _upload_p4(dev):
    dev.upload(_genes(4, LENGTHS_P4))
    for c in range(3):
        assert dev.class_kernel_name(c) != '', c
    return dev


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a, t=ctypes.c_int64):
    return a.ctypes.data_as(ctypes.POINTER(t))


def test_refusals_leave_the_handle_as_it_was(three_classes):
    lib = _lib.load()
    dev = _upload_p4(_lib.Device(0))
    n, p, h = dev.n, dev.p, dev.h
    first = _run(dev)

    scale, rho, flags = _scale(p), np.zeros((n, p)), np.zeros(n, np.int32)
    ds = np.zeros(n, np.int64)

    def iteration(key, nmf_iter=5, bins=20, min_hc=50, rate=1, scale=scale, ds=None, rho=None, flags=None):
        prm = _lib.Params(nmf_iter, bins, min_hc, rate, 0, 1)
        rc = lib.dn_baseline_iteration(h, _dp(scale), ctypes.byref(prm), None if ds is None else _ip(ds),
                                       None if rho is None else _dp(rho), None if flags is None else _ip(flags, ctypes.c_int32), None)
        _api_errors.refused(lib, rc, key, live=(h, p))

    iteration('params.nmf_iter', nmf_iter=0)
    iteration('params.bins', bins=65)
    iteration('params.min_high_coverage', min_hc=1)
    iteration('params.downsample_rate', rate=0)
    iteration('params.ds_start_null', rate=2)
    iteration('params.rate_too_large', rate=min(LENGTHS_P4) + 50, ds=ds)
    bad_ds = ds.copy()
    bad_ds[n // 2] = 2
    iteration('params.ds_start_range', rate=2, ds=bad_ds)
    zero = scale.copy()
    zero[1] = 0.0
    iteration('baseline_iteration.scale', scale=zero)
    iteration('baseline_iteration.rho_flags', rho=rho)

    vec = np.zeros(3 * p + 4)
    _api_errors.refused(lib, lib.dn_outer_partials(h, _dp(vec)), 'outer_partials.state', live=(h, p))
    _api_errors.refused(lib, lib.dn_outer_apply(h, None, _dp(scale), 0), 'outer_apply.state', live=(h, p))
    _api_errors.refused(lib, lib.dn_init_partials(h, _dp(vec)), 'init_partials.state', live=(h, p))
    _api_errors.refused(lib, lib.dn_comm_allreduce(h, _dp(vec), 4), 'comm_allreduce.state', live=(h, p))

    rows = np.array([0, n], np.int64)
    _api_errors.refused(lib, lib.dn_fetch_rows(h, rows.size, _ip(rows), _dp(rho), _ip(flags, ctypes.c_int32)), 'fetch_rows.range', live=(h, p))
    out = np.zeros(p * sum(LENGTHS_P4))
    for ids, key in (([1, 1], 'fetch_estimates_subset.duplicate'), ([0, n], 'fetch_estimates_subset.range')):
        ids = np.array(ids, np.int64)
        _api_errors.refused(lib, lib.dn_fetch_estimates_subset(h, ids.size, _ip(ids), _dp(out)), key, live=(h, p))

    mats = [np.ascontiguousarray(g, dtype=np.float64) for g in _genes(p, LENGTHS_P4[:2])]
    ptrs = (ctypes.c_void_p * 2)(*[m.ctypes.data for m in mats])
    lengths = np.array([m.shape[1] for m in mats], np.int64)
    K, E, status = np.zeros(2 * p), np.zeros(int(lengths.sum())), np.zeros(2, np.int32)
    rc = lib.dn_nmf_f64(h, 2, p, ptrs, _ip(lengths), 7, 5, _dp(K), _dp(E), None, _ip(status, ctypes.c_int32))
    _api_errors.refused(lib, rc, 'nmf_f64.mode', live=(h, p))
    prm = _lib.Params(0, 20, 50, 1, 0, 0)
    rc = lib.dn_baseline_selection_f64(h, 2, p, ptrs, _ip(lengths), ctypes.byref(prm), None, _dp(rho), _ip(flags, ctypes.c_int32), None, None)
    _api_errors.refused(lib, rc, 'params.nmf_iter', live=(h, p))

    # the test seam: refused for its arguments on this handle, for its state on one that holds no data set
    _api_errors.refused(lib, lib.dn_debug_plant(h, 0, None), 'debug_plant.null', live=(h, p))
    for which in (-1, 6):
        _api_errors.refused(lib, lib.dn_debug_plant(h, which, rho.ctypes.data), 'debug_plant.which', live=(h, p))
    _api_errors.refused(lib, lib.dn_debug_peek(h, 0, None), 'debug_peek.null', live=(h, p))
    for which in (-1, 2):
        _api_errors.refused(lib, lib.dn_debug_peek(h, which, rho.ctypes.data), 'debug_peek.which', live=(h, p))
    empty = _lib.Device(0)
    _api_errors.refused(lib, lib.dn_debug_plant(empty.h, 0, rho.ctypes.data), 'debug_plant.state', live=(h, p))
    _api_errors.refused(lib, lib.dn_debug_peek(empty.h, 0, rho.ctypes.data), 'debug_peek.state', live=(h, p))
    empty.close()

    _same(_run(dev), first)
    dev.close()


def test_every_refusal_of_an_uploaded_or_empty_handle_is_made():
    """The keys of the two tables that need a device all appear in this file (the host file holds the early ones)."""
    text = open(__file__).read()
    for key in list(_api_errors.UPLOADED) + list(_api_errors.EMPTY):
        assert repr(key) in text, key


def test_reuse_and_teardown_with_three_live_classes(three_classes):
    dev = _upload_p4(_lib.Device(0))
    got4 = _run(dev)
    dev.upload(_genes(10, LENGTHS_P10))
    got10 = _run(dev)
    dev.close()

    fresh = _upload_p4(_lib.Device(0))
    _same(got4, _run(fresh))
    fresh.close()
    fresh = _lib.Device(0).upload(_genes(10, LENGTHS_P10))
    _same(got10, _run(fresh))
    fresh.close()
