"""ctypes binding of the C ABI declared in include/isochrones_amd_nested.h (libiso_nested.so, nested sampling of a
catalog); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _nested_cabi.IsoError)
from ._sidelib import SideLibrary

MAX_BANDS = 12
MAX_D = 7
EXPORTED_SYMBOLS = ("iso_nested_version", "iso_nested_last_error", "iso_nested_last_kernel", "iso_nested_fast_args_size",
                    "iso_nested_remove", "iso_nested_max_live", "iso_nested_max_live_catalog", "iso_nested_fit")


def _declare(L):
    vp, i64, ci, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    L.iso_nested_last_kernel.restype = C.c_char_p
    L.iso_nested_last_kernel.argtypes = []
    L.iso_nested_fast_args_size.restype = C.c_size_t
    L.iso_nested_fast_args_size.argtypes = []
    L.iso_nested_remove.restype = ci
    L.iso_nested_remove.argtypes = [ci, ci]
    L.iso_nested_max_live.restype = ci
    L.iso_nested_max_live.argtypes = [ci, ci, ci]
    L.iso_nested_max_live_catalog.restype = ci
    L.iso_nested_max_live_catalog.argtypes = [vp, C.c_size_t, ci, ci]
    L.iso_nested_fit.restype = ci
    L.iso_nested_fit.argtypes = [vp, C.c_size_t, ci, ci, ci, i64, vp, ci, dbl, dbl, C.c_uint64, ci, ci, ci, vp, vp, vp, ci,
                                 vp, vp, ci, vp]


_SIDE = SideLibrary("nested", "nested-sampling", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
