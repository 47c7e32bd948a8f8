"""ctypes binding of the C ABI declared in include/isochrones_amd_cluster.h (libiso_cluster.so, the star-cluster
likelihood); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _cluster_cabi.IsoError)
from ._sidelib import SideLibrary

MAX_BANDS = 32
MAX_PROPS = 8
EXPORTED_SYMBOLS = ("iso_cluster_version", "iso_cluster_last_error", "iso_cluster_lnlike")


def _declare(L):
    vp, i64 = C.c_void_p, C.c_int64
    L.iso_cluster_lnlike.restype = C.c_int
    L.iso_cluster_lnlike.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp]


_SIDE = SideLibrary("cluster", "cluster", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
