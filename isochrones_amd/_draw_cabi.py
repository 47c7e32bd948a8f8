"""ctypes binding of the C ABI declared in include/isochrones_amd_draw.h (libiso_draw.so, the random draws of synthetic
populations and injection sets); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._cabi import IsoError  # noqa: F401  (callers catch it as _draw_cabi.IsoError)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
MAX_COLS = 8
MAX_BINS = 64
NPAR = 10
PHILOX_TAG = 0xD7
MAX_BLOCKS = 4096
FLAT, FLATLOG, POWERLAW, GAUSS, LOGNORMAL, CHABRIER, FEH, TRUNCGAUSS, LINGAUSS, TABLE, CONSTANT = range(1, 12)
EXPORTED_SYMBOLS = ("iso_draw_version", "iso_draw_last_error", "iso_draw_systems", "iso_draw_systems_host",
                    "iso_draw_uniforms_host")

#: ``iso_draw_record`` as a numpy structured type
RECORD = np.dtype([("kind", np.int32), ("parent", np.int32), ("stream", np.int32), ("reserved", np.int32),
                   ("lo", np.float64), ("hi", np.float64), ("p", np.float64, (NPAR,))], align=True)


def _declare(L):
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    for fn in (L.iso_draw_systems, L.iso_draw_systems_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, i32, vp, vp, i64, C.c_uint64, i32, i64, vp, i64, vp, vp]
    L.iso_draw_uniforms_host.restype = C.c_int
    L.iso_draw_uniforms_host.argtypes = [C.c_uint64, i32, vp, i64, i32, vp]


_SIDE = SideLibrary("draw", "random draws", _declare, label="draw")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
