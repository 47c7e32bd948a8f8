"""Host side of the exact (mass, age, [Fe/H]) -> EEP solve: what is computed once per table before libiso_solve.so
inverts a column along its last axis (include/isochrones_amd_solve.h), and the device-resident copy of it.

``column_ranges`` finds, per (i, j), the first and last finite index of the column and whether a NaN lies between them,
and checks that the column is nondecreasing along the last axis: a blend with nonnegative weights of nondecreasing
columns is nondecreasing, which is what lets the kernel bisect.  numpy only: it runs (and refuses a table) without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import functools

from . import _solve_cabi, _tables, device as dev
from .interp import HOST_CALL_ROWS


def column_ranges(col, name="column"):
    """``range[n0, n1, 2]`` (int32) of a NaN-padded ``col[n0, n1, nk]``: first finite index (with
    ``_solve_cabi.HOLE_BIT`` set when a non-finite entry lies inside the range) and last finite index; (nk, -1) for a
    column without a finite entry.  Raises ``ValueError`` naming the first (i, j, k) where the column decreases."""
    col = np.asarray(col, dtype=float)
    if col.ndim != 3:
        raise ValueError("column_ranges needs a [n0, n1, nk] array")
    nk = col.shape[2]
    fin = np.isfinite(col)
    with np.errstate(invalid="ignore"):
        # between finite neighbours only: padding and holes (NaN or inf) are no steps, columns with one walk the range
        down = (np.diff(col, axis=2) < 0) & fin[:, :, 1:] & fin[:, :, :-1]
    if down.any():
        i, j, k = (int(v) for v in np.argwhere(down)[0])
        raise ValueError("solve_eep needs '%s' nondecreasing along the last axis of the table, but at (i, j, k) = "
                         "(%d, %d, %d) it falls from %r to %r; use the Nelder-Mead path for this table "
                         "(get_eep(..., accurate=True) / get_eep_accurate)" % (name, i, j, k + 1, col[i, j, k], col[i, j, k + 1]))
    some = fin.any(axis=2)
    first = np.where(some, fin.argmax(axis=2), nk)
    last = np.where(some, nk - 1 - fin[:, :, ::-1].argmax(axis=2), -1)
    holes = some & (fin.sum(axis=2) != last - first + 1)
    out = np.empty(col.shape[:2] + (2,), dtype=np.int32)
    out[..., 0] = first | np.where(holes, _solve_cabi.HOLE_BIT, 0)
    out[..., 1] = last
    return out


class DeviceTable:
    """One column, its axes and ranges resident on a device, with the ``iso_solve_table`` that points at them."""

    def __init__(self, col, axes, ranges, device):
        import torch
        self.device = device
        self.col, self.axes, shape = _tables.pack_grid(col, axes, functools.partial(dev.to_device_f64, device=device))
        self.ranges = torch.as_tensor(np.ascontiguousarray(ranges, dtype=np.int32), device=torch.device("cuda", device))
        self.table = _tables.fill(_solve_cabi.IsoSolveTable, self.col, self.axes + [self.ranges], shape)

    def solve_device(self, x0, x1, target):
        """Contiguous float64 CUDA tensors of equal length on this device -> CUDA tensor, on the current stream."""
        out = dev.empty_f64((x0.numel(),), self.device)
        _solve_cabi.check(_solve_cabi.lib().iso_solve_last_axis(C.byref(self.table), dev.ptr(x0), dev.ptr(x1), dev.ptr(target),
                                                                x0.numel(), dev.ptr(out), dev.stream_ptr(self.device)))
        return out

    def solve_host(self, x0, x1, target):
        """Contiguous float64 host arrays of equal length -> numpy array; small batches go through the library's host
        entry point (one staging buffer, one launch, one wait), large ones through ``solve_device``."""
        n = x0.size
        if n > HOST_CALL_ROWS:
            return self.solve_device(*[dev.to_device_f64(x, self.device) for x in (x0, x1, target)]).cpu().numpy()
        out = np.empty(n)
        if n:
            stage = dev.empty_f64((4 * n,), self.device)
            _solve_cabi.check(_solve_cabi.lib().iso_solve_last_axis_host(
                C.byref(self.table), x0.ctypes.data, x1.ctypes.data, target.ctypes.data, n, out.ctypes.data,
                dev.ptr(stage), dev.stream_ptr(self.device)))
        return out
