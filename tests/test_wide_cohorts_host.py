"""
Wide cohorts (65 .. 256 samples), host side: what can be asked of the library without a GPU.  dn_p_max() is the new query;
dn_p_supported keeps its meaning (the count-path families of 2 .. 64 samples) and its answers.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p_max_is_exported_and_declared_and_p_supported_is_unchanged():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    from degnorm_amd import _lib, build
    build.build_library()                      # hipcc cross-compiles gfx950 without a GPU
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert 'dn_p_max' in ge.header_symbols()
    lib.dn_p_max.restype = ctypes.c_int
    assert lib.dn_p_max() == 256
    assert _lib.p_max() == 256
    assert lib.dn_p_supported(1) == 0
    for p in list(range(2, 13)) + [50, 64]:
        assert lib.dn_p_supported(p) == 1
    assert lib.dn_p_supported(65) == 0
    with open(os.path.join(ROOT, 'include', 'degnorm_amd.h')) as f:
        header = f.read()
    assert 'int  dn_p_max(void);' in header and '2 <= p <= dn_p_max()' in header
