"""ctypes binding of the C ABI declared in include/isochrones_amd_relation.h (libiso_relation.so, the hierarchical population
likelihood for a density that links one column to another); loaded by :mod:`isochrones_amd._sidelib`.  The records and the
column descriptors are ``_hier_cabi.RECORD`` and ``_hier_cabi.IsoHierColumn``."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _relation_cabi.IsoError)
from ._hier_cabi import MAX_COLS, RECORD, IsoHierColumn  # noqa: F401  (the library reads the hierarchical library's as they are)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
LINGAUSS = 9
ROW_TILE = 8
EXPORTED_SYMBOLS = ("iso_relation_version", "iso_relation_last_error", "iso_relation_lnlike", "iso_relation_lnlike_host",
                    "iso_relation_lnpdf_host")


def _declare(L):
    vp = C.c_void_p
    for fn in (L.iso_relation_lnlike, L.iso_relation_lnlike_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoHierColumn), C.c_int32, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.iso_relation_lnpdf_host.restype = C.c_int
    L.iso_relation_lnpdf_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int64, vp]


_SIDE = SideLibrary("relation", "linked population likelihood", _declare, label="relation")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
