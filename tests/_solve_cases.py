"""TEST INFRASTRUCTURE - the reference goldens of the exact EEP solve and small hand-built tables, one per rule of
include/isochrones_amd_solve.h, shared by the CPU tests of the twin and the GPU tests of the kernel."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "solve")

#: 10 x the largest |e_twin - e_reference| measured on the CPU per file (tests/golden/solve/README.md): the margin covers
#: Nelder-Mead's termination, which looks at the size of its simplex
GOLDEN_MAX_DIFF = {"track": 4.08e-11, "iso": 3.47e-11}
GOLDEN_TOL = {k: 10.0 * v for k, v in GOLDEN_MAX_DIFF.items()}

AX0 = np.array([0.0, 1.0, 2.0])
AX1 = np.array([10.0, 20.0, 40.0])
AXK = np.array([100.0, 101.0, 102.0, 104.0, 105.0, 106.0])
NAN = float("nan")


def golden(kind):
    """(grid, axes, column number, x0, x1, target, reference EEP, reference residual) of one fixture."""
    d = np.load(os.path.join(GOLDEN, kind + ".npz"))
    axes = (d["ax0"], d["ax1"], d["ax2"])
    icol = list(d["columns"]).index(str(d["column"]))
    x0, x1, y = (d["feh"], d["mass"], d["age"]) if kind == "track" else (d["age"], d["feh"], d["mass"])
    return d["grid"], axes, icol, x0, x1, y, d["eep"], d["resid"]


def table(profile, edits=()):
    """grid[3, 3, 6, 1]: every column is ``profile`` shifted by 0.25 i + 0.5 j (binary fractions: blends at cell
    midpoints are exact), then ``edits`` = ((i, j, k, value), ...) applied."""
    g = np.empty((3, 3, 6, 1))
    for i in range(3):
        for j in range(3):
            g[i, j, :, 0] = np.asarray(profile, dtype=float) + 0.25 * i + 0.5 * j
    for i, j, k, v in edits:
        g[i, j, k, 0] = v
    return g, (AX0, AX1, AXK)


PLATEAU = [1.0, 2.0, 2.0, 2.0, 3.0, 4.0]
RAMP = [1.0, 2.0, 3.0, 5.0, 6.0, 7.0]

#: name -> (profile, edits, [(x0, x1, target, expected)]); expected None: "whatever the twin says" is not allowed here -
#: every expectation is worked out by hand from the header's rules
CASES = {
    # on a node of both axes the cell above it enters: corners (0..1, 0..1), weights (1, 0, 0, 0)
    "plateau_smallest_eep": (PLATEAU, (), [(0.0, 10.0, 2.0, 101.0), (0.0, 10.0, 2.5, 104.5), (0.0, 10.0, 1.5, 100.5),
                                            (0.5, 15.0, 2.375, 101.0)]),
    "first_knot": (RAMP, (), [(0.0, 10.0, 1.0, 100.0), (0.0, 10.0, 0.5, NAN), (1.0, 20.0, 1.75, 100.0),
                              (0.0, 10.0, 7.0, 106.0), (0.0, 10.0, 7.5, NAN)]),
    "nan_and_off_axis": (RAMP, (), [(NAN, 10.0, 2.0, NAN), (0.0, NAN, 2.0, NAN), (0.0, 10.0, NAN, NAN),
                                    (-0.5, 10.0, 2.0, NAN), (2.5, 10.0, 2.0, NAN), (0.0, 9.0, 2.0, NAN),
                                    (0.0, 41.0, 2.0, NAN)]),
    # a NaN at (1, 1, 3): g(2) and g(3) are NaN in the four cells around (1, 1); below the hole the solve still works
    "hole_inside_range": (RAMP, ((1, 1, 3, NAN),), [(0.0, 10.0, 1.5, 100.5), (0.0, 10.0, 2.0, 101.0),
                                                   (0.0, 10.0, 2.5, NAN), (0.0, 10.0, 5.5, NAN),
                                                   (0.0, 10.0, 6.5, 105.5), (1.5, 30.0, 5.5 + 1.125, NAN)]),
    # the last node of ax0 / ax1 belongs to the cell below it (t = 1): column (1, 0) is short, so at (2, 10) g stops where it
    # does, and g(3) reads its padding; the cells at x1 = 40 hold full columns only
    "last_node": (RAMP, ((1, 0, 4, NAN), (1, 0, 5, NAN)),
                  [(2.0, 10.0, 1.5 + 0.5, 100.5), (2.0, 10.0, 3.0 + 0.5, 102.0), (2.0, 10.0, 4.0 + 0.5, NAN),
                   (2.0, 10.0, 6.5 + 0.5, NAN), (0.0, 40.0, 6.5 + 1.0, 105.5), (2.0, 40.0, 6.5 + 1.5, 105.5)]),
}
