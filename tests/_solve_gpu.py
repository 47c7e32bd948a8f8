"""iso_solve_last_axis and iso_solve_last_axis_host called through ctypes on a plain ``col[n0, n1, nk]`` and three axes:
what tests/test_gpu_solve.py and tests/test_gpu_solve_edges.py share."""
import ctypes as C

import numpy as np

from isochrones_amd import _solve_cabi, solve
from tests import _solve_twin as T

SENTINEL = -7.0
GUARD = 256                                                   # doubles behind every array: one whole workgroup of lanes


def _device_table(col, axes):
    from isochrones_amd import device as dev
    col = np.ascontiguousarray(col, dtype=float)
    return solve.DeviceTable(col, axes, solve.column_ranges(col), dev.current_device())


def device(col, axes, x0, x1, y, stream=None):
    """The kernel on host arrays copied to the device -> e as a numpy array.  ``stream``: a torch stream to copy, launch
    and wait on (the current one otherwise).  out lies in front of GUARD doubles of SENTINEL, which have to stay so, and
    every input in front of GUARD NaNs: a lane one past n reads NaN, and what it writes is seen here."""
    import torch
    from isochrones_amd import device as dev
    n = np.asarray(x0).size
    with torch.cuda.stream(stream):
        table = _device_table(col, axes)
        ins = [torch.as_tensor(np.concatenate([np.asarray(v, dtype=float).ravel(), np.full(GUARD, np.nan)]), device="cuda")
               for v in (x0, x1, y)]
        out = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        _solve_cabi.check(_solve_cabi.lib().iso_solve_last_axis(C.byref(table.table), dev.ptr(ins[0]), dev.ptr(ins[1]),
                                                                dev.ptr(ins[2]), n, dev.ptr(out), dev.stream_ptr(None)))
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        assert bool((out[n:] == SENTINEL).all()), "the kernel wrote behind the end of out"
        return out[:n].cpu().numpy()


def host(col, axes, x0, x1, y):
    """iso_solve_last_axis_host on the same arrays with a staging buffer of 4 n doubles, whatever n is."""
    import torch
    from isochrones_amd import device as dev
    table = _device_table(col, axes)
    xs = [np.ascontiguousarray(v, dtype=float).ravel() for v in (x0, x1, y)]
    n = xs[0].size
    stage = torch.full((4 * n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    out = np.full(n + GUARD, SENTINEL)
    _solve_cabi.check(_solve_cabi.lib().iso_solve_last_axis_host(C.byref(table.table), xs[0].ctypes.data, xs[1].ctypes.data,
                                                                 xs[2].ctypes.data, n, out.ctypes.data, dev.ptr(stage),
                                                                 dev.stream_ptr(None)))
    assert bool((stage[4 * n:] == SENTINEL).all()), "the host entry point wrote behind the end of its staging buffer"
    assert (out[n:] == SENTINEL).all(), "the host entry point wrote behind the end of out"
    return out[:n].copy()


def _hex(v):
    return "%r (%s)" % (float(v), float(v).hex() if np.isfinite(v) else "-")


def same(got, want, case=None):
    """NaN at the same positions and every other value the same 64 bits; raises AssertionError naming the first query
    that differs.  ``case`` = (col, axes, x0, x1, target) adds that query's inputs, cell, F, L and hole flag."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(got)
    bad = (nan != np.isnan(want)) | (~nan & (got.view(np.int64) != want.view(np.int64)))
    if not bad.any():
        return True
    q = int(np.flatnonzero(bad)[0])
    msg = "%d of %d results differ; first at query %d: got %s, want %s" % (bad.sum(), bad.size, q, _hex(got[q]), _hex(want[q]))
    if case is not None:
        col, axes, x0, x1, y = case
        ok, i, j, F, L = T.cell_ranges(col, axes, x0[q:q + 1], x1[q:q + 1])
        i, j = int(i[0]), int(j[0])
        flag = any(not np.isfinite(c[np.isfinite(c).argmax():c.size - np.isfinite(c)[::-1].argmax()]).all()
                   for c in (col[i, j], col[i, j + 1], col[i + 1, j], col[i + 1, j + 1]) if np.isfinite(c).any())
        msg += "; x0 = %s, x1 = %s, target = %s, inside %s, cell (%d, %d), F = %d, L = %d, hole flag %s" % (
            _hex(x0[q]), _hex(x1[q]), _hex(y[q]), bool(ok[0]), i, j, int(F[0]), int(L[0]), flag)
    raise AssertionError(msg)
