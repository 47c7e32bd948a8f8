"""ctypes binding of the C ABI declared in include/isochrones_amd_binfit.h (libiso_binfit.so, the moments of the stars'
posterior cell probabilities under a binned population density: expected counts per cell and their pair sums); loaded by
:mod:`isochrones_amd._sidelib`.  The limit of a grid is ``_binned_cabi``'s."""
from __future__ import annotations

import ctypes as C

from ._binned_cabi import MAX_CELLS  # noqa: F401  (the grid is the binned library's)
from ._cabi import IsoError  # noqa: F401  (callers catch it as _binfit_cabi.IsoError)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
CHUNK = 4096
TILE = 64
EXPORTED_SYMBOLS = ("iso_binfit_version", "iso_binfit_last_error", "iso_binfit_workspace_doubles", "iso_binfit_moments",
                    "iso_binfit_moments_host")


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    L.iso_binfit_workspace_doubles.restype = C.c_int64
    L.iso_binfit_workspace_doubles.argtypes = [i32, i32, i32, C.c_int]
    for fn in (L.iso_binfit_moments, L.iso_binfit_moments_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]


_SIDE = SideLibrary("binfit", "binned maximum-likelihood moments", _declare, label="binfit")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
