"""ctypes binding of the C ABI declared in include/isochrones_amd_nested.h (libiso_nested.so, nested sampling of a
catalog).  Like :func:`isochrones_amd._cabi.lib`, torch is imported before the library is opened, so that both libraries
bind to the HIP runtime torch bundles.  There is no CPU fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError

MAX_BANDS = 12
MAX_D = 7
EXPORTED_SYMBOLS = ("iso_nested_version", "iso_nested_last_error", "iso_nested_last_kernel", "iso_nested_fast_args_size",
                    "iso_nested_remove", "iso_nested_max_live", "iso_nested_max_live_catalog", "iso_nested_fit")

_LIB = None


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_nested.so")


def lib():
    """Load (once) and return libiso_nested.so with argtypes set."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IsoError("isochrones_amd: nested-sampling library not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(path)
    vp, i64, ci, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    for name in ("iso_nested_version", "iso_nested_last_error", "iso_nested_last_kernel"):
        getattr(L, name).restype = C.c_char_p
        getattr(L, name).argtypes = []
    L.iso_nested_fast_args_size.restype = C.c_size_t
    L.iso_nested_fast_args_size.argtypes = []
    L.iso_nested_remove.restype = ci
    L.iso_nested_remove.argtypes = [ci, ci]
    L.iso_nested_max_live.restype = ci
    L.iso_nested_max_live.argtypes = [ci, ci, ci]
    L.iso_nested_max_live_catalog.restype = ci
    L.iso_nested_max_live_catalog.argtypes = [vp, C.c_size_t, ci, ci]
    L.iso_nested_fit.restype = ci
    L.iso_nested_fit.argtypes = [vp, C.c_size_t, ci, ci, ci, i64, vp, ci, dbl, dbl, C.c_uint64, ci, ci, ci, vp, vp, vp, ci,
                                 vp, vp, ci, vp]
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().iso_nested_last_error()
        e = IsoError("isochrones_amd nested C-ABI error %d: %s" % (rc, (msg or b"").decode()))
        e.rc = rc
        raise e
