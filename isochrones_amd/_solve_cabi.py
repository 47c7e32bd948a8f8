"""ctypes binding of the C ABI declared in include/isochrones_amd_solve.h (libiso_solve.so, the exact
(mass, age, [Fe/H]) -> EEP solve).  Like :func:`isochrones_amd._cabi.lib`, torch is imported before the library is opened,
so that every library binds to the HIP runtime torch bundles.  There is no CPU fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError

HOLE_BIT = 0x40000000
EXPORTED_SYMBOLS = ("iso_solve_version", "iso_solve_last_error", "iso_solve_last_axis", "iso_solve_last_axis_host")

_LIB = None


class IsoSolveTable(C.Structure):
    """``iso_solve_table``: device pointers of one prepared table and its shape."""
    _fields_ = [("col", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("range", C.c_void_p), ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32)]


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_solve.so")


def lib():
    """Load (once) and return libiso_solve.so with argtypes set."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IsoError("isochrones_amd: solve library not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(path)
    vp, i64, tp = C.c_void_p, C.c_int64, C.POINTER(IsoSolveTable)
    L.iso_solve_version.restype = C.c_char_p
    L.iso_solve_version.argtypes = []
    L.iso_solve_last_error.restype = C.c_char_p
    L.iso_solve_last_error.argtypes = []
    L.iso_solve_last_axis.restype = C.c_int
    L.iso_solve_last_axis.argtypes = [tp, vp, vp, vp, i64, vp, vp]
    L.iso_solve_last_axis_host.restype = C.c_int
    L.iso_solve_last_axis_host.argtypes = [tp, vp, vp, vp, i64, vp, vp, vp]
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().iso_solve_last_error()
        e = IsoError("isochrones_amd solve C-ABI error %d: %s" % (rc, (msg or b"").decode()))
        e.rc = rc
        raise e
