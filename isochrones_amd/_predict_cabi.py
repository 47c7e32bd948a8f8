"""ctypes binding of the C ABI declared in include/isochrones_amd_predict.h (libiso_predict.so, the posterior-predictive
check of a stored chain).  Like :func:`isochrones_amd._cabi.lib`, torch is imported before the library is opened, so that every
library binds to the HIP runtime torch bundles.  There is no fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError

ERR_INVALID = -1
ERR_HIP = -2
MAX_BANDS = 32
MAX_COMPS = 3
NSPEC = 4
LANES = 128
EXPORTED_SYMBOLS = ("iso_predict_version", "iso_predict_last_error", "iso_predict_chain", "iso_predict_chain_host")

_LIB = None


class IsoPredictModelTable(C.Structure):
    """``iso_predict_model_table``: (Teff, logg, feh, Mbol) packed ``[n0][n1][nk][4]`` and its axes."""
    _fields_ = [("cols", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32), ("reserved", C.c_int32)]


class IsoPredictBcTable(C.Structure):
    """``iso_predict_bc_table``: B band columns packed ``[nT][ng][nf][nA][B]`` and the four axes."""
    _fields_ = [("bc", C.c_void_p), ("axT", C.c_void_p), ("axg", C.c_void_p), ("axf", C.c_void_p), ("axA", C.c_void_p),
                ("nT", C.c_int32), ("ng", C.c_int32), ("nf", C.c_int32), ("nA", C.c_int32), ("B", C.c_int32),
                ("reserved", C.c_int32)]


class IsoPredictOut(C.Structure):
    """``iso_predict_out``: the outputs of one call, a null pointer skips one."""
    _fields_ = [("mags", C.c_void_p), ("term_chi2", C.c_void_p), ("ppc", C.c_void_p), ("n_bad", C.c_void_p),
                ("map_index", C.c_void_p), ("map_pars", C.c_void_p), ("mag_nan", C.c_void_p)]


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_predict.so")


def lib():
    """Load (once) and return libiso_predict.so with argtypes set."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IsoError("isochrones_amd: posterior-predictive library not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (there is no fallback)" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    L.iso_predict_version.restype = C.c_char_p
    L.iso_predict_version.argtypes = []
    L.iso_predict_last_error.restype = C.c_char_p
    L.iso_predict_last_error.argtypes = []
    for fn in (L.iso_predict_chain, L.iso_predict_chain_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoPredictModelTable), C.POINTER(IsoPredictBcTable), vp, vp, C.c_int, C.c_int64, i32, i32,
                       i32, i32, i32, C.POINTER(i32), i32, i32, i32, vp, vp, C.POINTER(IsoPredictOut), vp]
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().iso_predict_last_error()
        e = IsoError("isochrones_amd predict C-ABI error %d: %s" % (rc, (msg or b"").decode()))
        e.rc = rc
        raise e
