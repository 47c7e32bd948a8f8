"""ctypes binding of the C ABI declared in include/isochrones_amd_binned.h (libiso_binned.so, the hierarchical population
likelihood for a density that is piecewise constant on a grid of bins); loaded by :mod:`isochrones_amd._sidelib`.  The
records and the column descriptors are ``_hier_cabi.RECORD`` and ``_hier_cabi.IsoHierColumn``."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _binned_cabi.IsoError)
from ._hier_cabi import MAX_COLS, RECORD, IsoHierColumn  # noqa: F401  (the library reads the hierarchical library's as they are)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_CELLS = 64
MAX_AXES = 2
ROW_TILE = 8
EXPORTED_SYMBOLS = ("iso_binned_version", "iso_binned_last_error", "iso_binned_compress", "iso_binned_compress_host",
                    "iso_binned_lnlike", "iso_binned_lnlike_host")


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    ip = C.POINTER(i32)
    for fn in (L.iso_binned_compress, L.iso_binned_compress_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoHierColumn), i32, C.c_int, C.c_int64, i32, i32, i32, i32, vp, vp, i32, ip, i32, ip, ip,
                       vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for fn in (L.iso_binned_lnlike, L.iso_binned_lnlike_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_int64, vp, i32, vp, vp, vp, vp, vp, vp]


_SIDE = SideLibrary("binned", "binned population likelihood", _declare, label="binned")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
