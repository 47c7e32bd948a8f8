"""ctypes binding of the C ABI declared in include/isochrones_amd_derived.h (libiso_derived.so, model-grid columns along a
stored chain); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _derived_cabi.IsoError)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_COLS = 8
MAX_COMPS = 3
EXPORTED_SYMBOLS = ("iso_derived_version", "iso_derived_last_error", "iso_derived_chain", "iso_derived_chain_host")


class IsoDerivedTable(C.Structure):
    """``iso_derived_table``: pointers of one packed table and its shape."""
    _fields_ = [("cols", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32), ("Q", C.c_int32)]


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    for fn in (L.iso_derived_chain, L.iso_derived_chain_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoDerivedTable), vp, C.c_int, C.c_int64, i32, i32, i32, i32, i32, C.POINTER(i32), i32,
                       vp, vp, vp]


_SIDE = SideLibrary("derived", "derived-properties", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
