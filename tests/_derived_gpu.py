"""iso_derived_chain and iso_derived_chain_host called through ctypes on numpy inputs: what tests/test_gpu_derived.py and
tests/test_gpu_derived_edges.py share."""
import ctypes as C

import numpy as np

from isochrones_amd import _derived_cabi
from tests import _derived_twin as tw

SENTINEL = -7


def _comps(comps):
    return (C.c_int32 * (3 * len(comps)))(*[i for comp in comps for i in comp])


def _guarded(torch, shape, dtype):
    """(the allocation, its leading view of ``shape``): SENTINEL everywhere, with room behind the view that has to stay so."""
    n = int(np.prod(shape))
    flat = torch.full((n + max(shape[-1] * shape[-2], 64),), SENTINEL, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def device(x, layout, S, W, cols, axes, comps, ens_begin=0, n_out=None, stream=None, cols_offset=0):
    """The kernel on host arrays copied to the device -> (out, nan_count) as numpy arrays; both start as SENTINEL.
    ``stream``: a torch stream to copy, launch and wait on (the current one otherwise).  ``cols_offset``: the table is
    placed that many doubles into its allocation, so that its pointer is 8-byte but not 16-byte aligned at 1.
    out and nan_count lie in front of a stretch of SENTINEL and the chain in front of one of NaN: a row index one past
    the range reads NaN, and what it writes is seen here."""
    import torch
    from isochrones_amd import device as dev
    n_out = S - ens_begin if n_out is None else n_out
    T = x.shape[0]
    ndim = x.shape[1] if layout == tw.PARAM_MAJOR else x.shape[2]
    with torch.cuda.stream(stream):
        flat = torch.empty(cols.size + cols_offset, dtype=torch.float64, device="cuda")
        d_cols = flat[cols_offset:]
        d_cols.copy_(torch.as_tensor(np.ascontiguousarray(cols).ravel()))
        assert d_cols.data_ptr() % 16 == 8 * (cols_offset % 2)
        d_x = torch.as_tensor(np.concatenate([np.asarray(x).ravel(), np.full(max(ndim, 64), np.nan)]), device="cuda")
        d_ax = [torch.as_tensor(a, device="cuda") for a in axes]
        table = _derived_cabi.IsoDerivedTable(d_cols.data_ptr(), d_ax[0].data_ptr(), d_ax[1].data_ptr(), d_ax[2].data_ptr(),
                                              *cols.shape)
        Cn, Q = len(comps), cols.shape[3]
        out_all, out = _guarded(torch, (T, Cn * Q, n_out * W), torch.float64)
        nan_all, nan_count = _guarded(torch, (n_out, Cn * Q), torch.int32)
        _derived_cabi.check(_derived_cabi.lib().iso_derived_chain(C.byref(table), dev.ptr(d_x), layout, T, S, W, ndim,
                                                                  ens_begin, n_out, _comps(comps), Cn, dev.ptr(out),
                                                                  dev.ptr(nan_count), dev.stream_ptr(0)))
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        assert bool((out_all[out.numel():] == SENTINEL).all()), "the kernel wrote behind the end of out"
        assert bool((nan_all[nan_count.numel():] == SENTINEL).all()), "the kernel wrote behind the end of nan_count"
        return out.cpu().numpy(), nan_count.cpu().numpy()


def host(x, layout, S, W, cols, axes, comps):
    """iso_derived_chain_host on the same arrays, all ensembles -> (out, nan_count)."""
    table = _derived_cabi.IsoDerivedTable(cols.ctypes.data, axes[0].ctypes.data, axes[1].ctypes.data, axes[2].ctypes.data,
                                          *cols.shape)
    Cn, Q = len(comps), cols.shape[3]
    ndim = x.shape[1] if layout == tw.PARAM_MAJOR else x.shape[2]
    out = np.empty((x.shape[0], Cn * Q, S * W))
    nan_count = np.empty((S, Cn * Q), dtype=np.int32)
    rc = _derived_cabi.lib().iso_derived_chain_host(C.byref(table), x.ctypes.data_as(C.c_void_p), layout, x.shape[0], S, W,
                                                    ndim, 0, S, _comps(comps), Cn, out.ctypes.data_as(C.c_void_p),
                                                    nan_count.ctypes.data_as(C.c_void_p), None)
    assert rc == 0
    return out, nan_count
