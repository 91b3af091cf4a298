"""
The refusals of the NMF C ABI (csrc/dn_api.hip), without a GPU: every entry point that turns away a null handle or a null
argument before it touches the device returns the code and leaves the exact dn_last_error() text recorded in _api_errors.py,
and a following successful call of an entry point of this unit (none of them clears the text) leaves that text in place.
"""
import ctypes

import numpy as np
import pytest

import _api_errors
from degnorm_amd import _lib


def _args(fn, **by_index):
    """One argument per entry of fn.argtypes: None for a pointer, 0 for a number, except the positions given as i<k>=value."""
    args = [None if hasattr(t, 'contents') else 0 for t in fn.argtypes]
    for k, v in by_index.items():
        args[int(k[1:])] = v
    return args


_F32 = np.zeros(4, np.float32)
_I64 = np.ones(2, np.int64)
_PTRS = (ctypes.c_void_p * 2)(_F32.ctypes.data, _F32.ctypes.data)

CASES = [
    ('dn_create', {}, 'create.out_null'),
    ('dn_set_downsample_hint', {'i1': 2}, 'null_handle'),
    ('dn_set_trace_columns', {'i1': 8}, 'null_handle'),
    ('dn_set_solver_step_cap', {'i1': 100}, 'null_handle'),
    ('dn_upload_packed', {}, 'upload_packed.null'),
    ('dn_upload_packed', {'i1': 2, 'i2': 2, 'i3': _F32.ctypes.data_as(ctypes.POINTER(ctypes.c_float))}, 'upload_packed.null'),   # lengths null
    ('dn_upload_packed', {'i1': 2, 'i2': 2, 'i3': _F32.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                          'i4': _I64.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))}, 'null_handle'),
    ('dn_upload_ragged', {}, 'upload_ragged.null'),
    ('dn_upload_ragged', {'i1': 2, 'i2': 2, 'i3': _PTRS}, 'upload_ragged.null'),                                            # lengths null
    ('dn_upload_ragged', {'i1': 2, 'i2': 2, 'i3': _PTRS, 'i4': _I64.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 'i5': 1},
     'null_handle'),
    ('dn_ratio_svd_sums', {}, 'ratio_svd_sums.state'),
    ('dn_baseline_iteration', {}, 'baseline_iteration.state'),
    ('dn_init_begin', {}, 'init_begin.state'),
    ('dn_init_partials', {}, 'init_partials.state'),
    ('dn_outer_begin_scaled', {'i2': 1}, 'outer_begin_scaled.state'),
    ('dn_outer_begin', {'i2': 1}, 'outer_begin.state'),
    ('dn_outer_partials', {}, 'outer_partials.state'),
    ('dn_outer_partials_device', {}, 'outer_partials_device.state'),
    ('dn_outer_apply', {}, 'outer_apply.state'),
    ('dn_comm_unique_id', {}, 'comm_unique_id.null'),
    ('dn_comm_create', {'i3': 1}, 'comm_create.null_handle'),
    ('dn_comm_allreduce', {'i2': 1}, 'comm_allreduce.state'),
    ('dn_init_allreduce', {}, 'init_allreduce.state'),
    ('dn_outer_allreduce', {}, 'outer_allreduce.state'),
    ('dn_fetch_outer', {}, 'fetch_outer.state'),
    ('dn_fetch_rows', {'i1': 1}, 'fetch_rows.state'),
    ('dn_fetch_estimates', {}, 'fetch_estimates.state'),
    ('dn_fetch_estimates_subset', {'i1': 1}, 'fetch_estimates_subset.state'),
    ('dn_nmf_f64', {'i1': 1, 'i2': 2}, 'nmf_f64.null_handle'),
    ('dn_baseline_selection_f64', {'i1': 1, 'i2': 2}, 'baseline_selection_f64.null_handle'),
    ('dn_class_tier_cols', {}, 'class_tier_cols.bad'),
    ('dn_class_lengths', {'i1': 10, 'i2': 1}, 'class_lengths.null'),
    ('dn_synchronize', {}, 'null_handle'),
    ('dn_debug_plant', {}, 'debug_plant.null_handle'),
    ('dn_debug_plant', {'i1': 9, 'i2': _F32.ctypes.data}, 'debug_plant.null_handle'),       # the handle is looked at first
    ('dn_debug_peek', {}, 'debug_peek.null_handle'),
    ('dn_debug_peek', {'i1': 9, 'i2': _F32.ctypes.data}, 'debug_peek.null_handle'),
]


@pytest.mark.parametrize('name,overrides,key', CASES, ids=['{0}-{1}'.format(k, c[0]) for k, c in enumerate(CASES)])
def test_refused_before_the_device(name, overrides, key):
    lib = _lib.load()
    fn = getattr(lib, name)
    _api_errors.refused(lib, fn(*_args(fn, **overrides)), key)


def test_every_early_refusal_of_the_table_is_made():
    assert sorted({c[2] for c in CASES}) == sorted(_api_errors.EARLY)


def test_probes_and_getters_of_a_null_handle_leave_the_text():
    lib = _lib.load()
    rc = lib.dn_synchronize(None)
    _api_errors.refused(lib, rc, 'null_handle')
    assert lib.dn_measure_read_gbps(None, 1 << 30, 1) == 0.0 and lib.dn_measure_copy_gbps(None, 1 << 30, 1) == 0.0
    assert lib.dn_last_kernel_ms(None) == 0.0 and lib.dn_last_f64_ms(None) == 0.0
    assert lib.dn_split_length(None) == 0 and lib.dn_tiny_length(None) == 0
    assert lib.dn_class_kernel_name(None, 0) == b'' and lib.dn_main_kernel_name(None) == b''
    assert lib.dn_last_error() == b'null handle'
