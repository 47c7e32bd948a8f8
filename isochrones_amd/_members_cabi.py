"""ctypes binding of the C ABI declared in include/isochrones_amd_members.h (libiso_members.so, the per-star moments of
the star-cluster likelihood's integrand); loaded by :mod:`isochrones_amd._sidelib`."""
from __future__ import annotations

import ctypes as C

from ._cabi import IsoError  # noqa: F401  (callers catch it as _members_cabi.IsoError)
from ._sidelib import SideLibrary

MAX_BANDS = 32
MAX_PROPS = 8
ISO_MEMBERS_NMOM = NMOM = 11
NINNER = 6
ERR_INVALID = -1
ERR_HIP = -2
#: the moments, in the header's order
MOMENTS = ("eep_A", "eep_A_sq", "mass_A", "mass_A_sq", "q", "q_sq", "mass_B", "mass_B_sq", "p_pair", "p_single", "q_x_pair")
EXPORTED_SYMBOLS = ("iso_members_version", "iso_members_last_error", "iso_members_moments", "iso_members_moments_host")


def _declare(L):
    vp, i64 = C.c_void_p, C.c_int64
    for fn in (L.iso_members_moments, L.iso_members_moments_host):
        fn.restype = C.c_int
        fn.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp]


_SIDE = SideLibrary("members", "cluster members", _declare)
library_path, lib, check = _SIDE.library_path, _SIDE.lib, _SIDE.check
