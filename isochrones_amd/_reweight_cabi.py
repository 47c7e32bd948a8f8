"""ctypes binding of the C ABI declared in include/isochrones_amd_reweight.h (libiso_reweight.so, the population-informed
posterior of every star from its stored chain); loaded by :mod:`isochrones_amd._sidelib`.  The records and the column
descriptors are ``_hier_cabi.RECORD`` and ``_hier_cabi.IsoHierColumn``."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _reweight_cabi.IsoError)
from ._hier_cabi import MAX_COLS, RECORD, IsoHierColumn  # noqa: F401  (the library reads the hierarchical library's as they are)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_VALUES = 8
MAX_PROBS = 8
ROW_TILE = 64
EXPORTED_SYMBOLS = ("iso_reweight_version", "iso_reweight_last_error", "iso_reweight_stars", "iso_reweight_stars_host",
                    "iso_reweight_summary", "iso_reweight_summary_host")


def _declare(L):
    vp, col = C.c_void_p, C.POINTER(IsoHierColumn)
    for fn in (L.iso_reweight_stars, L.iso_reweight_stars_host):
        fn.restype = C.c_int
        fn.argtypes = [col, C.c_int32, col, C.c_int32, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       vp, vp, C.c_int32, vp, vp, C.POINTER(C.c_double), C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for fn in (L.iso_reweight_summary, L.iso_reweight_summary_host):
        fn.restype = C.c_int
        fn.argtypes = [col, C.c_int32, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp,
                       C.POINTER(C.c_double), C.c_int32, vp, vp, vp, vp, vp, vp]


_SIDE = SideLibrary("reweight", "star reweighting", _declare, label="reweight")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
