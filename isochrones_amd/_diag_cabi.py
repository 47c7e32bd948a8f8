"""ctypes binding of the C ABI declared in include/isochrones_amd_diag.h (libiso_diag.so, per-star chain convergence
diagnostics).  Like :func:`isochrones_amd._cabi.lib`, torch is imported before the library is opened, so that every
library binds to the HIP runtime torch bundles.  There is no fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError

NOUT = 5
TAU, WINDOW, WINDOW_OK, ESS, RHAT = range(NOUT)
DEFAULT_C = 5.0
DEFAULT_MAX_LAG = 1024
EXPORTED_SYMBOLS = ("iso_diag_version", "iso_diag_last_error", "iso_diag_chain", "iso_diag_chain_host")

_LIB = None


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_diag.so")


def lib():
    """Load (once) and return libiso_diag.so with argtypes set."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IsoError("isochrones_amd: diagnostics library not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (there is no fallback)" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(path)
    vp = C.c_void_p
    L.iso_diag_version.restype = C.c_char_p
    L.iso_diag_version.argtypes = []
    L.iso_diag_last_error.restype = C.c_char_p
    L.iso_diag_last_error.argtypes = []
    for fn in (L.iso_diag_chain, L.iso_diag_chain_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, vp]
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().iso_diag_last_error()
        e = IsoError("isochrones_amd diagnostics C-ABI error %d: %s" % (rc, (msg or b"").decode()))
        e.rc = rc
        raise e
