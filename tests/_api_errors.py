"""
The refusals of the NMF C ABI (csrc/dn_api.hip) that need no failing HIP call: return code and exact dn_last_error() text, as
the library gave them before its entry points were put under the exit rule of dn_host.hpp.  test_api_errors_host.py makes
the calls that are refused before the device is touched, test_gpu_api_exit_rule.py those that need an uploaded handle or an
empty one.  The test seam (dn_debug_plant, dn_debug_peek) has its rows in all three tables.
"""
import ctypes

from degnorm_amd import _lib

INVALID, STATE = _lib.DN_E_INVALID, _lib.DN_E_STATE

# null handle or null argument, refused before anything touches the device
EARLY = {
    'create.out_null': (INVALID, b'dn_create: out is null'),
    'null_handle': (INVALID, b'null handle'),
    'upload_packed.null': (INVALID, b'dn_upload_packed: null argument'),
    'upload_ragged.null': (INVALID, b'dn_upload_ragged: null argument'),
    'ratio_svd_sums.state': (STATE, b'dn_ratio_svd_sums: nothing uploaded'),
    'baseline_iteration.state': (STATE, b'dn_baseline_iteration: nothing uploaded'),
    'init_begin.state': (STATE, b'dn_init_begin: nothing uploaded'),
    'init_partials.state': (STATE, b'dn_init_partials: dn_init_begin has not been called'),
    'outer_begin_scaled.state': (STATE, b'dn_outer_begin_scaled: dn_init_begin has not been called'),
    'outer_begin.state': (STATE, b'dn_outer_begin: nothing uploaded'),
    'outer_partials.state': (STATE, b'dn_outer_partials: dn_outer_begin has not been called'),
    'outer_partials_device.state': (STATE, b'dn_outer_partials_device: dn_outer_begin has not been called'),
    'outer_apply.state': (STATE, b'dn_outer_apply: dn_outer_begin has not been called'),
    'comm_unique_id.null': (INVALID, b'dn_comm_unique_id: null argument'),
    'comm_create.null_handle': (INVALID, b'dn_comm_create: null handle'),
    'comm_allreduce.state': (STATE, b'dn_comm_allreduce: dn_comm_create has not been called'),
    'init_allreduce.state': (STATE, b'dn_init_allreduce: dn_comm_create has not been called'),
    'outer_allreduce.state': (STATE, b'dn_outer_allreduce: dn_comm_create has not been called'),
    'fetch_outer.state': (STATE, b'dn_fetch_outer: dn_outer_begin has not been called'),
    'fetch_rows.state': (STATE, b'dn_fetch_rows: nothing uploaded'),
    'fetch_estimates.state': (STATE, b'dn_fetch_estimates: nothing uploaded'),
    'fetch_estimates_subset.state': (STATE, b'dn_fetch_estimates_subset: nothing uploaded'),
    'nmf_f64.null_handle': (STATE, b'dn_nmf_f64: null handle'),
    'baseline_selection_f64.null_handle': (STATE, b'dn_baseline_selection_f64: null handle'),
    'class_tier_cols.bad': (INVALID, b'dn_class_tier_cols: bad argument'),
    'class_lengths.null': (INVALID, b'dn_class_lengths: null argument'),
    'debug_plant.null_handle': (INVALID, b'dn_debug_plant: null handle'),
    'debug_peek.null_handle': (INVALID, b'dn_debug_peek: null handle'),
}
# arguments and state of an uploaded handle; its state refusals repeat texts of EARLY
UPLOADED = {
    'params.nmf_iter': (INVALID, b'nmf_iter must be >= 1'),
    'params.bins': (INVALID, b'bins must be in [1, 64]'),
    'params.min_high_coverage': (INVALID, b'min_high_coverage must be >= 2 (nmf.py:34)'),
    'params.downsample_rate': (INVALID, b'downsample_rate must be >= 1'),
    'params.ds_start_null': (INVALID, b'downsample_rate > 1 needs per-gene start offsets'),
    'params.rate_too_large': (INVALID, b'downsample_rate is too large; take-every size > at least one gene.'),
    'params.ds_start_range': (INVALID, b'ds_start out of [0, rate)'),
    'baseline_iteration.scale': (INVALID, b'scale factors must be positive and finite'),
    'baseline_iteration.rho_flags': (INVALID, b'dn_baseline_iteration: rho and flags are fetched together or not at all'),
    'fetch_rows.range': (INVALID, b'dn_fetch_rows: row out of range'),
    'fetch_estimates_subset.duplicate': (INVALID, b'dn_fetch_estimates_subset: duplicate gene id'),
    'fetch_estimates_subset.range': (INVALID, b'dn_fetch_estimates_subset: gene id out of range'),
    'nmf_f64.mode': (INVALID, b'dn_nmf_f64: unknown mode'),
    'debug_plant.null': (INVALID, b'dn_debug_plant: null source'),
    'debug_plant.which': (INVALID, b'dn_debug_plant: unknown array'),
    'debug_peek.null': (INVALID, b'dn_debug_peek: null destination'),
    'debug_peek.which': (INVALID, b'dn_debug_peek: unknown array'),
}
# state of a handle that exists but holds no data set (a fresh one, or one whose upload was refused)
EMPTY = {
    'debug_plant.state': (STATE, b'dn_debug_plant: nothing uploaded'),
    'debug_peek.state': (STATE, b'dn_debug_peek: nothing uploaded'),
}
TABLE = dict(EARLY, **UPLOADED)
TABLE.update(EMPTY)


def refused(lib, rc, key, live=None):
    """Assert that a call which returned rc was refused with the code and text recorded under `key`, and that successful
    calls of entry points that do not clear the text (all of dn_api.hip) leave it in place: the null-handle no-ops, and, given
    `live` = (handle, number of samples) of an uploaded device, calls that do their work on it."""
    code, text = TABLE[key]
    assert rc == code, (key, rc, lib.dn_last_error())
    assert lib.dn_last_error() == text, key
    assert lib.dn_destroy(None) == _lib.DN_OK and lib.dn_comm_destroy(None) == _lib.DN_OK
    assert lib.dn_comm_size(None) == 0
    if live is not None:
        h, p = live
        row, rho, flag = ctypes.c_int64(0), (ctypes.c_double * p)(), ctypes.c_int32(0)
        reg, lds = ctypes.c_int32(0), ctypes.c_int32(0)
        assert lib.dn_synchronize(h) == _lib.DN_OK
        assert lib.dn_fetch_rows(h, 1, ctypes.byref(row), rho, ctypes.byref(flag)) == _lib.DN_OK      # queues a kernel and two copies
        assert lib.dn_class_tier_cols(h, 0, ctypes.byref(reg), ctypes.byref(lds)) == _lib.DN_OK
    assert lib.dn_last_error() == text, key
