"""ctypes binding of the C ABI declared in include/isochrones_amd_derived.h (libiso_derived.so, model-grid columns along a
stored chain).  Like :func:`isochrones_amd._cabi.lib`, torch is imported before the library is opened, so that every
library binds to the HIP runtime torch bundles.  There is no fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError

ERR_INVALID = -1
ERR_HIP = -2
MAX_COLS = 8
MAX_COMPS = 3
EXPORTED_SYMBOLS = ("iso_derived_version", "iso_derived_last_error", "iso_derived_chain", "iso_derived_chain_host")

_LIB = None


class IsoDerivedTable(C.Structure):
    """``iso_derived_table``: pointers of one packed table and its shape."""
    _fields_ = [("cols", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32), ("Q", C.c_int32)]


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_derived.so")


def lib():
    """Load (once) and return libiso_derived.so with argtypes set."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IsoError("isochrones_amd: derived-properties library not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (there is no fallback)" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    L.iso_derived_version.restype = C.c_char_p
    L.iso_derived_version.argtypes = []
    L.iso_derived_last_error.restype = C.c_char_p
    L.iso_derived_last_error.argtypes = []
    for fn in (L.iso_derived_chain, L.iso_derived_chain_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoDerivedTable), vp, C.c_int, C.c_int64, i32, i32, i32, i32, i32, C.POINTER(i32), i32,
                       vp, vp, vp]
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().iso_derived_last_error()
        e = IsoError("isochrones_amd derived C-ABI error %d: %s" % (rc, (msg or b"").decode()))
        e.rc = rc
        raise e
