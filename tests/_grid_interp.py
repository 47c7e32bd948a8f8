"""What tests/test_grid_interp_cpu.py and tests/test_gpu_grid_interp.py share: one packed table, 257 points, and the same
cell asked of two libraries - libiso_derived.so (one ensemble, one step, a row-major chain) and libiso_population.so
(``cols_out`` of single systems)."""
import functools

import numpy as np

from tests import _derived_twin as dtw, _population_twin as ptw

N = 257                     # one full 256-lane workgroup plus one lane
QS = (4, 5, 8)              # the even pair-load width, an odd width, the widest both libraries accept
MIN_FINITE_ROWS = 200
COMPS = [(0, 1, 2)]


@functools.lru_cache(maxsize=None)
def points():
    """[N, 3] coordinates over the axes of :func:`tests._population_twin.tables`: per axis its first and last node, one
    ulp outside either end and a NaN, the others fixed on the grid; then uniform draws over the cool part of the table.
    Read-only."""
    _, ax3, _, _, _ = ptw.tables(4, 1)
    f, m, e = ax3
    rng = np.random.default_rng(257)
    rows = np.column_stack([rng.uniform(f[0], f[-1], N), rng.uniform(0.5, 1.6, N), rng.uniform(e[0], e[-1], N)])
    good, n = [f[2] + 0.1, 0.85, e[10] + 0.3], 0
    for a, ax in enumerate(ax3):
        for x in (ax[0], ax[-1], np.nextafter(ax[0], -np.inf), np.nextafter(ax[-1], np.inf), np.nan):
            rows[n] = good
            rows[n, a] = x
            n += 1
    rows.setflags(write=False)
    return rows


def as_chain(rows):
    """The points as a stored chain of one ensemble of N walkers and one step, row-major: [1, N, 3]."""
    return np.ascontiguousarray(rows[None])


def as_systems(rows):
    """The points as N single systems: (coords [1, 3, N], distance [N], AV [N])."""
    return np.ascontiguousarray(rows.T[None]), np.full(len(rows), 100.0), np.full(len(rows), 0.1)


def assert_same_cell(derived_out, population_cols):
    """derived ``out`` [1, Q, N] against population ``cols_out`` [1, Q, N]: the same bit patterns, NaN positions included,
    over inputs of which enough are on the grid that a run of NaNs cannot pass for agreement."""
    a, b = np.ascontiguousarray(derived_out[0]), np.ascontiguousarray(population_cols[0])
    assert a.shape == b.shape == (a.shape[0], N)
    assert int(np.isfinite(a).all(axis=0).sum()) >= MIN_FINITE_ROWS
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    assert dtw.same_bits(a, b)
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
