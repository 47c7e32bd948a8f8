"""ctypes binding of the C ABI declared in include/isochrones_amd_predict.h (libiso_predict.so, the posterior-predictive
check of a stored chain); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _predict_cabi.IsoError)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_BANDS = 32
MAX_COMPS = 3
NSPEC = 4
LANES = 128
MAX_BLOCKS = 2048
EXPORTED_SYMBOLS = ("iso_predict_version", "iso_predict_last_error", "iso_predict_chain", "iso_predict_chain_host")


class IsoPredictModelTable(C.Structure):
    """``iso_predict_model_table``: (Teff, logg, feh, Mbol) packed ``[n0][n1][nk][4]`` and its axes."""
    _fields_ = [("cols", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32), ("reserved", C.c_int32)]


#: a BC table of the C ABI (this library's and libiso_population.so's): B band columns packed ``[nT][ng][nf][nA][B]`` and
#: the four axes
BC_TABLE_FIELDS = [("bc", C.c_void_p), ("axT", C.c_void_p), ("axg", C.c_void_p), ("axf", C.c_void_p), ("axA", C.c_void_p),
                   ("nT", C.c_int32), ("ng", C.c_int32), ("nf", C.c_int32), ("nA", C.c_int32), ("B", C.c_int32),
                   ("reserved", C.c_int32)]


class IsoPredictBcTable(C.Structure):
    """``iso_predict_bc_table``."""
    _fields_ = BC_TABLE_FIELDS


class IsoPredictOut(C.Structure):
    """``iso_predict_out``: the outputs of one call, a null pointer skips one."""
    _fields_ = [("mags", C.c_void_p), ("term_chi2", C.c_void_p), ("ppc", C.c_void_p), ("n_bad", C.c_void_p),
                ("map_index", C.c_void_p), ("map_pars", C.c_void_p), ("mag_nan", C.c_void_p)]


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    for fn in (L.iso_predict_chain, L.iso_predict_chain_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoPredictModelTable), C.POINTER(IsoPredictBcTable), vp, vp, C.c_int, C.c_int64, i32, i32,
                       i32, i32, i32, C.POINTER(i32), i32, i32, i32, vp, vp, C.POINTER(IsoPredictOut), vp]


_SIDE = SideLibrary("predict", "posterior-predictive", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
