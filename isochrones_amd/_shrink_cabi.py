"""ctypes binding of the C ABI declared in include/isochrones_amd_shrink.h (libiso_shrink.so, the population-informed
posterior and the bin memberships of every star under a binned population density); loaded by
:mod:`isochrones_amd._sidelib`.  The records and the column descriptors are ``_hier_cabi.RECORD`` and
``_hier_cabi.IsoHierColumn``, the limits of a grid ``_binned_cabi``'s."""
from __future__ import annotations

import ctypes as C

from ._binned_cabi import MAX_AXES, MAX_CELLS  # noqa: F401  (the grid is the binned library's)
from ._cabi import IsoError  # noqa: F401  (callers catch it as _shrink_cabi.IsoError)
from ._hier_cabi import MAX_COLS, RECORD, IsoHierColumn  # noqa: F401  (the library reads the hierarchical library's as they are)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
CELL_TILE = 2
EXPORTED_SYMBOLS = ("iso_shrink_version", "iso_shrink_last_error", "iso_shrink_cells", "iso_shrink_cells_host",
                    "iso_shrink_weights", "iso_shrink_weights_host")


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    ip = C.POINTER(i32)
    for fn in (L.iso_shrink_cells, L.iso_shrink_cells_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    for fn in (L.iso_shrink_weights, L.iso_shrink_weights_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoHierColumn), i32, C.c_int, C.c_int64, i32, i32, i32, i32, vp, vp, i32, ip, i32, ip, ip,
                       vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]


_SIDE = SideLibrary("shrink", "binned star reweighting", _declare, label="shrink")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
