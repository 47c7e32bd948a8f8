"""ctypes binding of the C ABI declared in include/isochrones_amd_diag.h (libiso_diag.so, per-star chain convergence
diagnostics); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _diag_cabi.IsoError)
from ._sidelib import SideLibrary

NOUT = 5
TAU, WINDOW, WINDOW_OK, ESS, RHAT = range(NOUT)
DEFAULT_C = 5.0
DEFAULT_MAX_LAG = 1024
EXPORTED_SYMBOLS = ("iso_diag_version", "iso_diag_last_error", "iso_diag_chain", "iso_diag_chain_host")


def _declare(L):
    vp = C.c_void_p
    for fn in (L.iso_diag_chain, L.iso_diag_chain_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, vp]


_SIDE = SideLibrary("diag", "diagnostics", _declare, label="diagnostics")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
