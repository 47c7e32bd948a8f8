"""The numpy twin of the N-D interpolation (tests/_interp_twin.py) against what the reference's DFInterpolator recorded for
the uniform-step edge tables (tests/golden/interp_edges.npz) and against the C oracle, and the conditions the GPU tests of
tests/test_gpu_interp_edges.py rely on, counted by the twin so that none of them can pass vacuously."""
import numpy as np
import pytest

from tests import _fixtures as fx
from tests import _interp_twin as tw

UNIFORM = list(tw.UNIFORM)
ALL = UNIFORM + list(tw.UNSTAGED) + list(tw.MINIMUM)


@pytest.fixture(scope="module")
def golden():
    return fx.load("interp_edges")


def _same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", UNIFORM)
def test_float64_twin_equals_the_reference_and_the_oracle(name, golden):
    from oracle import oracle as orc
    t = tw.edge_table(name)
    pts, want = golden[name + "_pts"], golden[name + "_vals"]
    # the fixture's probes are the table's, without those on the last node of an axis (the reference reads past the table)
    keep = np.ones(t.probes.shape[0], dtype=bool)
    for d, a in enumerate(t.axes):
        keep &= ~(t.probes[:, d] == a[-1])
    assert np.array_equal(pts, t.probes[keep], equal_nan=True) and 600 < pts.shape[0] < 4000
    xs = [np.ascontiguousarray(pts[:, d]) for d in range(t.nd)]
    icols = np.arange(t.ncol)
    got, _ = tw.interp(t.grid, t.axes, xs, icols, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern of the twin differs from the reference's"
    assert _same(got, want), "the float64 twin does not reproduce the reference bit for bit"
    o = orc.OracleTable(t.grid, t.axes).interp(xs, icols)
    assert np.array_equal(np.isnan(o), np.isnan(want))
    fx.assert_close(o, want, 1e-13, atol=1e-14, what="oracle, " + name)
    # the reference itself is within the bound of the long-double twin
    assert tw.check(want, t.grid, t.axes, xs, icols, "reference, " + name) <= 1.0


@pytest.mark.parametrize("name", UNIFORM)
def test_uniform_tables_have_decisive_fixup_probes(name):
    t = tw.edge_table(name)
    for a in t.axes:
        assert tw.is_uniform(a) and 20 <= a.size <= 300 and float(a[1]) not in (0.25, 0.5, 1.0, 2.0)
    for guess in (tw.first_guess_generic, tw.first_guess_fused):
        up, down = tw.fixup_counts(t, guess)
        print("%s %s: decisive ++ %d, -- %d" % (name, guess.__name__, up, down))
        assert up >= 3 and down >= 3, (name, guess.__name__, up, down)


def test_is_uniform_restates_the_library():
    assert tw.is_uniform(np.arange(64) * 0.3) and tw.is_uniform(np.arange(5.0, 50.0)) and tw.is_uniform([0.0, 1e-3])
    assert not tw.is_uniform([0.0, 0.3, 0.6, 0.95]) and not tw.is_uniform([1.0]) and not tw.is_uniform([-2.0, 1e-17])
    assert not tw.is_uniform(0.1 + np.arange(40) * 0.3)          # i*step + a0 rounds twice: not the stored linspace-like nodes
    # the counts the tables were designed from (a_i = i*0.3, n = 64; nodes and their two neighbours)
    a = np.arange(64) * 0.3
    x = np.clip(np.concatenate([a, np.nextafter(a, -np.inf), np.nextafter(a, np.inf)]), a[0], a[-1])
    for guess in (tw.first_guess_generic, tw.first_guess_fused):
        d = tw.fixup_needed(a, x, guess)
        assert (d == 1).sum() >= 3 and (d == -1).sum() >= 3


@pytest.mark.parametrize("name", ALL)
def test_tables_are_mostly_finite_and_float64_keeps_the_bound(name):
    t = tw.edge_table(name)
    icols = np.arange(t.ncol)
    got, _ = tw.interp(t.grid, t.axes, t.xs(), icols, dtype=np.float64)
    assert np.isfinite(got).mean() > 0.5, np.isfinite(got).mean()
    assert np.isnan(got).any()
    worst = tw.check(got, t.grid, t.axes, t.xs(), icols, name)
    print("%s: float64 twin error / limit %.3g" % (name, worst))
    # every kind of probe is there: nodes, neighbours, one ulp outside, NaN
    for d, a in enumerate(t.axes):
        x = t.probes[:, d]
        assert np.isnan(x).any() and (x == a[0]).any() and (x == a[-1]).any()
        assert (x == np.nextafter(a[0], -np.inf)).any() and (x == np.nextafter(a[-1], np.inf)).any()


def test_staging_of_the_unstaged_tables():
    want = {"G2_global": ([-1, 0], 3), "G2_exact": ([0, 6141], 6144), "G3_global": ([0, 6000, -1], 6002),
            "G3_exact": ([0, 6140, 6142], 6144)}
    for name, w in want.items():
        assert tw.staged_doubles(tw.edge_table(name).axes) == w, name
        a = tw.edge_table(name).axes[0]
        assert (np.diff(a) == np.spacing(a[:-1])).sum() >= 40      # nodes one ulp apart
    for name in tw.MINIMUM:
        assert all(a.size == 2 for a in tw.edge_table(name).axes)


def test_neighbour_marks_a_probe_next_to_a_nan_node():
    t = tw.edge_table("U2")
    m = t.nan_nodes[0][0]
    a = t.axes[0]
    xs = [np.array([a[m - 1], a[m - 3]]), np.array([t.axes[1][2] * 1.01] * 2)]
    _, dec = tw.neighbour(t.grid, t.axes, xs, np.arange(t.ncol), 0, -1)
    assert dec.tolist() == [True, False]


def test_the_grid_cap_of_the_header_is_the_one_the_tests_read():
    """One trip of k_interp's wave-stride loop is ISO_MAX_GRID_BLOCKS workgroups of four waves; the GPU tests read the cap
    from the ctypes module, which mirrors the public header."""
    import os
    import re
    from isochrones_amd import _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "isochrones_amd.h")).read()
    assert int(re.search(r"#define\s+ISO_MAX_GRID_BLOCKS\s+(\d+)", header).group(1)) == _cabi.ISO_MAX_GRID_BLOCKS
    assert tw.MAX_LDS_AXIS_DOUBLES == 6144               # read from the library's sources: what the G tables were sized for


def test_the_fused_guess_on_the_axis_of_the_fused_cases():
    """a_i = 0.7 i, i = 0 .. 999 (the EEP axis of the fused GPU cases): the library calls it uniform; the generic guess is off
    in both directions, the fused one only ever too low (its reciprocal rounds down) - at the nodes and their neighbours no
    probe needs the fused bracket's --k on this axis.  a_i = 0.1 i is the mirror image, which is why the GPU file adds it."""
    for step, fused_up, fused_down in ((0.7, True, False), (0.1, False, True)):
        a = np.arange(1000) * step
        assert tw.is_uniform(a)
        x = np.clip(np.concatenate([a, np.nextafter(a, -np.inf), np.nextafter(a, np.inf)]), a[0], a[-1])
        g, f = tw.fixup_needed(a, x, tw.first_guess_generic), tw.fixup_needed(a, x, tw.first_guess_fused)
        assert (g == 1).sum() >= 3 and (g == -1).sum() >= 3
        assert ((f == 1).sum() >= 3) == fused_up and ((f == -1).sum() >= 3) == fused_down
        assert ((f == 1).sum() == 0) == (not fused_up) and ((f == -1).sum() == 0) == (not fused_down)
