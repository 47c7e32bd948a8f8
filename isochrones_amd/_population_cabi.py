"""ctypes binding of the C ABI declared in include/isochrones_amd_population.h (libiso_population.so, a batch of coeval
single or binary systems evaluated on the model and the BC grid); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _population_cabi.IsoError)
from ._predict_cabi import BC_TABLE_FIELDS
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_COLS = 32
MAX_BANDS = 32
MAX_COMPS = 2
MAX_BLOCKS = 2048
EXPORTED_SYMBOLS = ("iso_population_version", "iso_population_last_error", "iso_population_eval",
                    "iso_population_eval_host")


class IsoPopulationModelTable(C.Structure):
    """``iso_population_model_table``: Q columns packed ``[n0][n1][nk][Q]``, the axes, and where (Teff, logg, feh, Mbol)
    are among the columns."""
    _fields_ = [("cols", C.c_void_p), ("ax0", C.c_void_p), ("ax1", C.c_void_p), ("axk", C.c_void_p),
                ("n0", C.c_int32), ("n1", C.c_int32), ("nk", C.c_int32), ("Q", C.c_int32), ("hot", C.c_int32 * 4)]


class IsoPopulationBcTable(C.Structure):
    """``iso_population_bc_table``: the same fields as ``iso_predict_bc_table``."""
    _fields_ = BC_TABLE_FIELDS


class IsoPopulationOut(C.Structure):
    """``iso_population_out``: the outputs of one call, a null pointer skips one."""
    _fields_ = [("cols_out", C.c_void_p), ("mag_out", C.c_void_p), ("A_out", C.c_void_p), ("sys_mag", C.c_void_p),
                ("sys_A", C.c_void_p)]


def _declare(L):
    vp = C.c_void_p
    for fn in (L.iso_population_eval, L.iso_population_eval_host):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(IsoPopulationModelTable), C.POINTER(IsoPopulationBcTable), vp, vp, vp, C.c_int64, C.c_int32,
                       C.POINTER(IsoPopulationOut), vp]


_SIDE = SideLibrary("population", "population", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
