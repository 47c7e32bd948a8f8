"""ctypes binding of the C ABI declared in include/isochrones_amd_cluster.h (libiso_cluster.so, the star-cluster
likelihood).  Like :func:`isochrones_amd._cabi.lib`, torch is imported before the library is opened, so that both libraries
bind to the HIP runtime torch bundles.  There is no CPU fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError

MAX_BANDS = 32
MAX_PROPS = 8
EXPORTED_SYMBOLS = ("iso_cluster_version", "iso_cluster_last_error", "iso_cluster_lnlike")

_LIB = None


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_cluster.so")


def lib():
    """Load (once) and return libiso_cluster.so with argtypes set."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IsoError("isochrones_amd: cluster library not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(path)
    vp, i64 = C.c_void_p, C.c_int64
    L.iso_cluster_version.restype = C.c_char_p
    L.iso_cluster_version.argtypes = []
    L.iso_cluster_last_error.restype = C.c_char_p
    L.iso_cluster_last_error.argtypes = []
    L.iso_cluster_lnlike.restype = C.c_int
    L.iso_cluster_lnlike.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp]
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().iso_cluster_last_error()
        e = IsoError("isochrones_amd cluster C-ABI error %d: %s" % (rc, (msg or b"").decode()))
        e.rc = rc
        raise e
