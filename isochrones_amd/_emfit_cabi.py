"""ctypes binding of the C ABI declared in include/isochrones_amd_emfit.h (libiso_emfit.so, a batch of weighted EM fits of
a binned population's cell masses with the loop on the device, and the star weights of a bootstrap); loaded by
:mod:`isochrones_amd._sidelib`.  The limit of a grid is ``_binned_cabi``'s."""
from __future__ import annotations

import ctypes as C

from ._binned_cabi import MAX_CELLS  # noqa: F401  (the grid is the binned library's)
from ._cabi import IsoError  # noqa: F401  (callers catch it as _emfit_cabi.IsoError)
from ._sidelib import SideLibrary

ERR_INVALID = -1
ERR_HIP = -2
RUNNING, CONVERGED, MAX_ITER, EMPTY = 0, 1, 2, 3
POISSON, EXP = 0, 1
LANES = 256
LAUNCH_WORK = 1 << 31
PHILOX_TAG = 0xB7
POISSON_TERMS = 18
EXPORTED_SYMBOLS = ("iso_emfit_version", "iso_emfit_last_error", "iso_emfit_run", "iso_emfit_run_host", "iso_emfit_weights",
                    "iso_emfit_weights_host")


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    for fn in (L.iso_emfit_run, L.iso_emfit_run_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, i32, C.c_double, i32, vp, vp, vp, vp, vp, vp, vp]
    for fn in (L.iso_emfit_weights, L.iso_emfit_weights_host):
        fn.restype = C.c_int
        fn.argtypes = [i32, C.c_uint64, i32, i32, i32, vp, vp]


_SIDE = SideLibrary("emfit", "batched EM fit", _declare, label="emfit")
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
