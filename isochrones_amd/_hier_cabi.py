"""ctypes binding of the C ABI declared in include/isochrones_amd_hier.h (libiso_hier.so, the hierarchical population
likelihood from the stored chains of a catalog); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._cabi import IsoError  # noqa: F401  (callers catch it as _hier_cabi.IsoError)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_COLS = 4
NPAR = 6
ROW_TILE = 8
FLAT, FLATLOG, POWERLAW, GAUSS, LOGNORMAL, CHABRIER, FEH, TRUNCGAUSS = range(1, 9)
EXPORTED_SYMBOLS = ("iso_hier_version", "iso_hier_last_error", "iso_hier_lnlike", "iso_hier_lnlike_host",
                    "iso_hier_lnpdf_host")

#: ``iso_hier_record`` as a numpy structured type: records are packed by the thousand, without a Python loop
RECORD = np.dtype([("kind", np.int32), ("reserved", np.int32), ("lo", np.float64), ("hi", np.float64),
                   ("p", np.float64, (NPAR,))], align=True)


class IsoHierColumn(C.Structure):
    """``iso_hier_column``: one value column where it lies in a stored or derived chain."""
    _fields_ = [("base", C.c_void_p), ("ncols", C.c_int32), ("col", C.c_int32), ("n_ens", C.c_int32), ("first", C.c_int32)]


def _declare(L):
    vp = C.c_void_p
    for fn in (L.iso_hier_lnlike, L.iso_hier_lnlike_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoHierColumn), C.c_int32, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.iso_hier_lnpdf_host.restype = C.c_int
    L.iso_hier_lnpdf_host.argtypes = [vp, C.c_int32, vp, C.c_int64, vp]


_SIDE = SideLibrary("hier", "hierarchical likelihood", _declare, label="hierarchical")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
