"""iso_hier_lnlike (k_hier_stars, k_hier_total) on the device against iso_hier_lnlike_host, within the limits of
tests/_hier_twin.py, on the smallest shapes at which the kernel can still go wrong: no full wavefront (M = 35), one
wavefront exactly, several passes of a workgroup over its star (M = 1200), H = 1, the row tile, tile + 1 and 3 tiles + 5,
Q = 1 and 4, both layouts, columns from two storages; S = 257 and 513 stars (more than the total's workgroup has threads);
every family kind; the -inf, NaN, masked and +-700 cases.  And bit
identity of a star's row alone, in a batch, in a sub-range of stars and in any tiling of the hyper rows."""
import numpy as np
import pytest

from isochrones_amd import _cabi, _hier_cabi as hc
from tests import _hier_twin as tw

pytestmark = pytest.mark.gpu
TILE = hc.ROW_TILE
PM, RM = _cabi.CHAIN_PARAM_MAJOR, _cabi.CHAIN_ROW_MAJOR


@pytest.fixture(scope="module")
def lib():
    return hc.lib()


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _against_host(lib, device, case, what):
    rc, host = tw.call(lib, case)
    assert rc == 0, lib.iso_hier_last_error()
    rc, got = tw.call(lib, case, device=device)
    assert rc == 0, lib.iso_hier_last_error()
    want = dict(host, rmax=tw.want(case)["rmax"])
    tw.assert_matches(host, tw.want(case), what)
    with np.errstate(invalid="ignore"):
        d = np.abs(got["ell"] - host["ell"])
    print(what, "max |d ell| = %.2e" % np.nanmax(np.where(np.isfinite(d), d, 0.0)))
    tw.assert_matches(got, want, what)
    return got


#          S, W,  T,  Q, H,            layout
SHAPES = [(3, 5,  7,  1, 1,            PM),         # M = 35: no wavefront is full
          (3, 5,  7,  4, 3 * TILE + 5, RM),
          (3, 5,  7,  4, TILE + 1,     PM),
          (3, 64, 1,  4, TILE,         PM),         # one wavefront exactly
          (3, 64, 1,  1, TILE + 1,     RM),
          (2, 40, 30, 1, TILE + 1,     PM),         # M = 1200: five passes, the last one partial
          (2, 40, 30, 4, 1,            RM),
          (2, 40, 30, 4, 3 * TILE + 5, PM)]


@pytest.mark.parametrize("S, W, T, Q, H, layout", SHAPES)
def test_device_matches_the_host_entry(lib, device, S, W, T, Q, H, layout):
    case = tw.random_case(S, W, T, Q, H, seed=7 * Q + H + W, layout=layout)
    assert Q == 1 or len({w[1] for w in case["where"]}) == 2         # columns from two storages with different C
    got = _against_host(lib, device, case, (S, W, T, Q, H, layout))
    assert np.isfinite(got["ell"]).all() and np.isfinite(got["L"]).all()


@pytest.mark.parametrize("kind", range(1, 9))
def test_every_kind_as_interim_and_as_population(lib, device, kind):
    _against_host(lib, device, tw.kind_case(kind), kind)


@pytest.mark.parametrize("name", ["no_support", "nan", "masked", "span_700"])
def test_special_cases(lib, device, name):
    case = tw.special_cases()[name]
    g = _against_host(lib, device, case, name)
    if name == "no_support":
        assert np.isneginf(g["ell"][0, 1]) and g["ess"][0, 1] == 0.0 and np.isneginf(g["L"][0]) and g["min_ess"][0] == 0.0
    elif name == "nan":
        assert list(g["n_bad"]) == [1, 0, 2]
    elif name == "masked":
        assert np.isnan(g["ell"][:, 1]).all() and np.isnan(g["ess"][:, 1]).all() and g["n_bad"][1] == 0
    else:
        assert tw.want(case)["rmax"].max() > 690 and np.isfinite(g["ell"]).all() and np.isfinite(g["ess"]).all()


BLOCK = 256                                                          # threads of k_hier_total's workgroup: a pass of row_total


@pytest.mark.parametrize("S", [BLOCK + 1, 2 * BLOCK + 1])
@pytest.mark.parametrize("masked", [False, True])
def test_the_row_total_takes_a_second_and_a_third_pass_over_the_stars(lib, device, S, masked):
    """More stars than the total's workgroup has threads: thread 0 adds a second star (S = 257) and a third (S = 513).
    With the stars 0 .. 255 masked every term of L and min_ess comes from the second and the third pass."""
    case = tw.random_case(S, 5, 7, 1, TILE + 1, seed=S)
    keep = np.ones(S, bool)
    if masked:
        keep[:BLOCK] = False
        case["mask"] = keep.astype(np.int32)
    rc, host = tw.call(lib, case)
    assert rc == 0, lib.iso_hier_last_error()
    rc, got = tw.call(lib, case, device=device, guard=True)
    assert rc == 0, lib.iso_hier_last_error()
    for k in ("ell", "ess", "n_bad", "L", "min_ess"):
        assert not (got[k] == -7).any(), k                           # (a masked star's ell and ess are written too: NaN)
    twin = tw.want(case)
    tw.assert_matches(host, twin, (S, masked, "host"))
    tw.assert_matches(got, twin, (S, masked, "device"))
    tw.assert_matches(got, dict(host, rmax=twin["rmax"]), (S, masked, "device against host"))
    assert np.isfinite(got["L"]).all() and np.isnan(got["ell"][:, ~keep]).all() and np.isfinite(got["ell"][:, keep]).all()
    # L and min_ess are the sum and the minimum of the device's own star terms
    own = got["ell"][:, keep].sum(axis=1)
    print("S = %d, masked %s: max |L - sum ell| / |sum ell| = %.2e" % (S, masked, np.max(np.abs(got["L"] - own) / np.abs(own))))
    assert np.array_equal(got["min_ess"], got["ess"][:, keep].min(axis=1))
    assert np.allclose(got["L"], own, rtol=1e-14, atol=0)


@pytest.fixture(scope="module")
def batch(lib, device):
    """seven stars, 29 rows, three columns from two storages, M = 1200; evaluated once"""
    case = tw.random_case(7, 40, 30, 3, 3 * TILE + 5, seed=11)
    rc, got = tw.call(lib, case, device=device)
    assert rc == 0, lib.iso_hier_last_error()
    return case, got


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_a_star_alone_in_a_batch_and_in_a_sub_range(lib, device, batch):
    case, whole = batch
    for s in (0, 3, 6):
        alone = tw.fixed_case(case["x"][:, s:s + 1], list(case["interim"][:, None]), [[row[q:q + 1] for q in range(len(row))] for row in case["rows"]],
                              40, 30, seed=50 + s)
        rc, one = tw.call(lib, alone, device=device)
        assert rc == 0 and _same(one["ell"][:, 0], whole["ell"][:, s]) and _same(one["ess"][:, 0], whole["ess"][:, s])
        assert one["n_bad"][0] == whole["n_bad"][s]
        rc, part = tw.call(lib, case, device=device, ens_begin=s, n_ens_out=1, total=False)
        assert rc == 0 and _same(part["ell"][:, s], whole["ell"][:, s]) and _same(part["ess"][:, s], whole["ess"][:, s])
        others = [i for i in range(7) if i != s]
        assert (part["ell"][:, others] == -7.0).all() and (part["n_bad"][others] == -7).all() and (part["L"] == -7.0).all()
    rc, part = tw.call(lib, case, device=device, ens_begin=2, n_ens_out=4, total=False)
    assert rc == 0 and _same(part["ell"][:, 2:6], whole["ell"][:, 2:6]) and _same(part["ess"][:, 2:6], whole["ess"][:, 2:6])


def test_a_row_alone_and_in_any_tiling(lib, device, batch):
    case, whole = batch
    H = case["rows"].shape[0]
    for sl in (slice(0, 1), slice(TILE, TILE + 1), slice(H - 1, H), slice(5, 20), slice(3, 3 + TILE), slice(1, H)):
        rc, got = tw.call(lib, case, device=device, rows=case["rows"][sl])
        assert rc == 0 and _same(got["ell"], whole["ell"][sl]) and _same(got["ess"], whole["ess"][sl]), sl
        assert _same(got["L"], whole["L"][sl]) and _same(got["min_ess"], whole["min_ess"][sl]), sl


def test_repeated_calls_and_another_storage_give_the_same_bits(lib, device, batch):
    case, whole = batch
    rc, again = tw.call(lib, case, device=device)
    assert rc == 0
    for k in ("L", "min_ess", "ell", "ess", "n_bad"):
        assert _same(again[k], whole[k]), k
    # the same columns in one storage of another width, and row-major
    for layout, split in ((PM, False), (RM, True)):
        st, where = tw.place(case["x"], 40, 30, layout, seed=99, split=split)
        assert layout != case["layout"] or [w[1:] for w in where] != [w[1:] for w in case["where"]]
        moved = dict(case, storages=st, where=where, layout=layout)
        rc, got = tw.call(lib, moved, device=device)
        assert rc == 0
        for k in ("L", "min_ess", "ell", "ess", "n_bad"):
            assert _same(got[k], whole[k]), (k, layout)
