"""ctypes binding of the C ABI declared in include/isochrones_amd_select.h (libiso_select.so, the detectable fraction of a
population density from an injection set); loaded by :mod:`isochrones_amd._sidelib`.  The records are ``_hier_cabi.RECORD``."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _select_cabi.IsoError)
from ._hier_cabi import MAX_COLS, RECORD, ROW_TILE  # noqa: F401  (the library reads iso_hier_record as it is)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
CHUNK = 4096
EXPORTED_SYMBOLS = ("iso_select_version", "iso_select_last_error", "iso_select_workspace_doubles", "iso_select_alpha",
                    "iso_select_alpha_host", "iso_select_lnpdf_host")


def _declare(L):
    vp = C.c_void_p
    L.iso_select_workspace_doubles.restype = C.c_int64
    L.iso_select_workspace_doubles.argtypes = [C.c_int64, C.c_int32]
    for fn in (L.iso_select_alpha, L.iso_select_alpha_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_int32, C.c_int64, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.iso_select_lnpdf_host.restype = C.c_int
    L.iso_select_lnpdf_host.argtypes = [vp, C.c_int32, vp, C.c_int64, vp]


_SIDE = SideLibrary("select", "selection effects", _declare, label="selection")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
