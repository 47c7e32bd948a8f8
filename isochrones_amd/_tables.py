"""The packed grids the side libraries read: columns of the model grid ``[n0, n1, nk, Q]`` and bands of the
bolometric-correction grid ``[nT, ng, nf, nA, B]``, contiguous float64 next to their axes, where ``put`` keeps arrays
(``dev.to_device_f64`` bound to a device, or a backend's ``array``), and the struct that points at them."""
from __future__ import annotations

import numpy as np


def pack_grid(grid, axes, put):
    """``grid`` made contiguous float64 and its ``axes`` through ``put``: (array, axes, shape)."""
    packed = np.ascontiguousarray(grid, dtype=np.float64)
    return put(packed), [put(a) for a in axes], packed.shape


def pack_model(interp, icols, put):
    """The columns ``icols`` of a model grid's interpolator: (``[n0, n1, nk, Q]`` array, axes, shape)."""
    return pack_grid(interp.grid[..., list(icols)], interp.index_columns, put)


def pack_bc(ic, bands, put):
    """The columns of ``bands`` of the BC grid of ``ic``: (``[nT, ng, nf, nA, B]`` array, axes, shape)."""
    b = ic.bc_grid.interp
    return pack_grid(b.grid[..., [int(i) for i in ic._band_cols(list(bands))]], b.index_columns, put)


def _address(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def fill(struct, array, axes, sizes, *rest):
    """``struct(pointer, the axes' pointers, *sizes, *rest)``: a table struct of the C ABI over what a packer returned."""
    return struct(_address(array), *[_address(a) for a in axes], *sizes, *rest)


def check_bands(ic, bands, max_bands):
    """``bands`` (None: the grid's own; a name: that one) as a tuple, refused when too many or not on the BC grid."""
    bands = tuple(ic.bands if bands is None else ((bands,) if isinstance(bands, str) else bands))
    if not 1 <= len(bands) <= max_bands:
        raise ValueError("1 to %d bands per call, got %d" % (max_bands, len(bands)))
    have = list(ic.bc_grid.interp.columns)
    for b in bands:
        if b not in have:
            raise ValueError("the bolometric-correction grid has no band %r" % (b,))
    return bands
