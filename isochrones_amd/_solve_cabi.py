"""ctypes binding of the C ABI declared in include/isochrones_amd_solve.h (libiso_solve.so, the exact
(mass, age, [Fe/H]) -> EEP solve); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _solve_cabi.IsoError)
from ._sidelib import SideLibrary

HOLE_BIT = 0x40000000
EXPORTED_SYMBOLS = ("iso_solve_version", "iso_solve_last_error", "iso_solve_last_axis", "iso_solve_last_axis_host")


class IsoSolveTable(C.Structure):
    """``iso_solve_table``: device pointers of one prepared table and its shape."""
    _fields_ = [("col", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("range", C.c_void_p), ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32)]


def _declare(L):
    vp, i64, tp = C.c_void_p, C.c_int64, C.POINTER(IsoSolveTable)
    L.iso_solve_last_axis.restype = C.c_int
    L.iso_solve_last_axis.argtypes = [tp, vp, vp, vp, i64, vp, vp]
    L.iso_solve_last_axis_host.restype = C.c_int
    L.iso_solve_last_axis_host.argtypes = [tp, vp, vp, vp, i64, vp, vp, vp]


_SIDE = SideLibrary("solve", "solve", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
