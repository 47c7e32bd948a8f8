"""The mixed-row cases of tests/_mixed_rows.py on the device: iso_hier_lnlike, iso_select_alpha, iso_reweight_stars and
iso_relation_lnlike against their host entries and the long-double twins, within the twins' own limits (tests/_hier_twin.py,
_select_twin.py, _reweight_twin.py, _relation_twin.py; quantiles exactly), with rows that differ inside one row tile: every
kind in every column of a tile, ln x needed by one tile and not by the next (and by the padding of a ragged tile alone),
supports that leave some rows of a tile dead and others not, and for the relation library linked and unlinked records in one
column of one tile, parents that differ by row, a linked last row repeated into the padding and one invalid parent among
valid ones.  tests/test_mixed_rows_cpu.py proves on the twins what each pattern is built for.

Shapes: S = 3 stars, (W, T) = (5, 7) and (257, 1), H = tile + 1 and 3 tiles + 5, both layouts (hier, relation); J = 37, 257
and CHUNK + 1 (select); S = 2, H = 65 and 150, V = 2, K = 3 (reweight).

Without a tolerance: a row's bits alone, in the whole table and in any slice of it; an unlinked row of a linked tile has
iso_hier_lnlike's bits (on the variant of the links pattern that links column 1 only, so that the whole row is unlinked);
a linked row has the bits of the same row where every row follows its parent; and at the edges of every kind's support
(lo, hi, one ulp outside, +-0, a negative value, +-inf, the smallest subnormal, the Chabrier break) at the first and last
lane of a wavefront, the last lane of the workgroup and the lone sample of the second pass: n_bad, -inf and NaN as the twin
has them and as counted by hand, weights of exactly 0 at bad samples, and nothing written outside the outputs."""
import numpy as np
import pytest

from isochrones_amd import _hier_cabi as hc, _relation_cabi as rl, _reweight_cabi as rc, _select_cabi as sc
from tests import _hier_twin as ht, _mixed_rows as mr, _relation_twin as rt, _reweight_twin as rw, _select_twin as st

pytestmark = pytest.mark.gpu
T8, T64, CHUNK = mr.T8, mr.T64, mr.CHUNK
SLICES = [(1, None), (T8 - 1, T8 + 1), (5, 20)]                    # the row slices [1, H), [T8 - 1, T8 + 1) and [5, 20)


@pytest.fixture(scope="module")
def libs():
    return dict(hier=hc.lib(), select=sc.lib(), reweight=rc.lib(), relation=rl.lib())


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _chain_against_host(mod, lib, device, case, what, guard=False):
    """``mod``: tests/_hier_twin.py with libiso_hier.so or tests/_relation_twin.py with libiso_relation.so"""
    code, host = mod.call(lib, case)
    assert code == 0, what
    code, got = mod.call(lib, case, device=device, guard=guard)
    assert code == 0, what
    twin = mod.want(case)
    mod.assert_matches(host, twin, what)
    print(what, "worst |d ell| over the limit: device - twin %.2e, device - host %.2e"
          % (mr.over_limit(got, twin), mr.over_limit(got, dict(host, rmax=twin["rmax"]))))
    mod.assert_matches(got, dict(host, rmax=twin["rmax"]), what)
    mod.assert_matches(got, twin, what)
    return got


def _select_against_host(lib, device, case, what, guard=False):
    code, host = st.call(lib, case)
    assert code == 0, lib.iso_select_last_error()
    code, got = st.call(lib, case, device=device, guard=guard)
    assert code == 0, lib.iso_select_last_error()
    twin = st.want(case)
    st.assert_matches(host, twin, what)
    print(what, "worst |d ln_alpha| over the limit: device - twin %.2e, device - host %.2e"
          % (mr.over_limit(got, twin, "ln_alpha", "tmax"), mr.over_limit(got, dict(host, tmax=twin["tmax"]), "ln_alpha", "tmax")))
    st.assert_matches(got, twin, what)
    st.assert_matches(got, dict(host, tmax=twin["tmax"]), what)
    return got


def _reweight_against_host(lib, device, case, what):
    code, host = rw.call(lib, case)
    assert code == 0, lib.iso_reweight_last_error()
    code, got = rw.call(lib, case, device=device)
    assert code == 0, lib.iso_reweight_last_error()
    twin = rw.want(case)
    rw.assert_matches(host, twin, what)
    print(what, "worst |d weight| over the limit: device - twin %.2e" % mr.over_limit_weights(got, twin))
    rw.assert_matches(got, twin, what)                              # quantiles exactly; no near tie in the case
    assert np.array_equal(got["quant"], host["quant"], equal_nan=True), what
    return got


# -- every pattern, every library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, W, T, H, layout", mr.CHAIN_SHAPES)
def test_hier(libs, device, name, W, T, H, layout):
    case = mr.chain_case(name, W, T, H, layout)
    got = _chain_against_host(ht, libs["hier"], device, case, ("hier", name, W, T, H, layout))
    assert np.array_equal(np.isneginf(got["ell"]), case["dead"] if name == "supports" else np.zeros((H, 3), bool))


@pytest.mark.parametrize("name, W, T, H, layout", mr.CHAIN_SHAPES)
def test_relation_on_unlinked_rows(libs, device, name, W, T, H, layout):
    case = mr.chain_case(name, W, T, H, layout)
    got = _chain_against_host(rt, libs["relation"], device, case, ("relation", name, W, T, H, layout))
    assert np.array_equal(np.isneginf(got["ell"]), case["dead"] if name == "supports" else np.zeros((H, 3), bool))


@pytest.mark.parametrize("H, W, T, layout", mr.LINK_SHAPES)
def test_relation_links(libs, device, H, W, T, layout):
    got = _chain_against_host(rt, libs["relation"], device, mr.links_case(H, W, T, layout), ("relation", "links", H, W, T, layout))
    assert np.isfinite(got["ell"]).all() and np.isfinite(got["L"]).all() and (got["n_bad"] == 0).all()


@pytest.mark.parametrize("reserved", [1, 4, -1])                   # itself, past Q, negative
def test_one_invalid_parent_in_the_middle_of_a_tile(libs, device, reserved):
    H, row = 2 * T8 + 3, T8 + 4
    good, bad = mr.links_case(H, 5, 7), mr.links_case(H, 5, 7, bad=(row, reserved))
    got = _chain_against_host(rt, libs["relation"], device, bad, ("relation", "bad parent", reserved), guard=True)
    code, ref = rt.call(libs["relation"], good, device=device)
    assert code == 0
    others = np.arange(H) != row
    assert np.isneginf(got["ell"][row]).all() and (got["ess"][row] == 0.0).all() and list(got["n_bad"]) == [0, 0, 0]
    assert np.isneginf(got["L"][row]) and got["min_ess"][row] == 0.0
    for k in ("ell", "ess", "L", "min_ess"):                        # every other row untouched
        assert got[k][others].tobytes() == ref[k][others].tobytes() and np.isfinite(got[k][others]).all()


@pytest.mark.parametrize("name, J, H", mr.SELECT_SHAPES)
def test_select(libs, device, name, J, H):
    case = mr.select_case(name, J, H)
    got = _select_against_host(libs["select"], device, case, ("select", name, J, H))
    assert got["n_bad"] == 0
    assert np.array_equal(np.isneginf(got["ln_alpha"]), case["dead"].all(axis=1) if name == "supports" else np.zeros(H, bool))


@pytest.mark.parametrize("name, W, T, H, layout", mr.REWEIGHT_SHAPES)
def test_reweight(libs, device, name, W, T, H, layout):
    case = mr.reweight_case(name, W, T, H, layout)
    got = _reweight_against_host(libs["reweight"], device, case, ("reweight", name, W, T, H, layout))
    assert (got["n_bad"] == 0).all() and (got["wsum"] > 0).all()


# -- a row in any company -----------------------------------------------------------------------------------------------
def _rows_alone_and_in_slices(call, rows, keys):
    """``call(rows) -> dict``; the results of the whole table, of each row alone and of the slices, compared in bytes"""
    H = rows.shape[0]
    whole = call(rows)
    for h in range(H):
        one = call(rows[h:h + 1])
        assert all(one[k][0].tobytes() == whole[k][h].tobytes() for k in keys), ("row alone", h)
    for a, b in SLICES:
        b = H if b is None else b
        assert b <= H
        part = call(rows[a:b])
        assert all(part[k].tobytes() == whole[k][a:b].tobytes() for k in keys), ("slice", a, b)


@pytest.mark.parametrize("name", ["kinds", "supports"])
@pytest.mark.parametrize("which", ["hier", "relation"])
def test_a_row_in_any_company(libs, device, which, name):
    mod = ht if which == "hier" else rt
    case = mr.chain_case(name, 5, 7, 3 * T8 + 5)

    def call(rows):
        code, got = mod.call(libs[which], case, device=device, rows=np.ascontiguousarray(rows), total=False)
        assert code == 0
        return got
    _rows_alone_and_in_slices(call, case["rows"], ("ell", "ess"))


@pytest.mark.parametrize("W, T", mr.WT)
def test_a_linked_row_in_any_company(libs, device, W, T):
    case = mr.links_case(3 * T8 + 5, W, T)

    def call(rows):
        code, got = rt.call(libs["relation"], case, device=device, rows=np.ascontiguousarray(rows), total=False)
        assert code == 0
        return got
    _rows_alone_and_in_slices(call, case["rows"], ("ell", "ess"))


@pytest.mark.parametrize("name, J", [("kinds", 257), ("supports", 257), ("supports", CHUNK + 1)])
def test_a_select_row_in_any_company(libs, device, name, J):
    case = mr.select_case(name, J, 3 * T8 + 5)

    def call(rows):
        code, got = st.call(libs["select"], case, device=device, rows=np.ascontiguousarray(rows))
        assert code == 0
        return got
    _rows_alone_and_in_slices(call, case["rows"], ("ln_alpha", "n_eff"))


# -- linked and unlinked rows of one tile ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W, T, layout", mr.LINK_SHAPES[:4])
def test_unlinked_rows_inside_linked_tiles_have_the_bits_of_the_hier_library(libs, device, H, W, T, layout):
    """The variant that links column 1 only: a row h % 3 == 2 is then unlinked in every column, and it goes through the
    second loop of k_relation_stars (its tile has linked rows in column 1) with k_hier_stars's arithmetic."""
    case = mr.links_case(H, W, T, layout, link3=False)
    par = mr.parent_of(case["rows"])
    assert (par[:, [0, 2, 3]] == -1).all() and (par[2::3, 1] == -1).all() and (par[0::3, 1] == 0).all() and (par[1::3, 1] == 2).all()
    code, rel = rt.call(libs["relation"], case, device=device, total=False)
    assert code == 0
    plain = case["rows"].copy()
    plain[par >= 0] = mr.flat(0.1, 10.0)[0]                         # any record iso_hier_lnlike accepts: those rows are not compared
    assert (plain["kind"] != rl.LINGAUSS).all() and plain[2::3].tobytes() == case["rows"][2::3].tobytes()
    code, hier = ht.call(libs["hier"], case, device=device, rows=plain, total=False)
    assert code == 0
    for k in ("ell", "ess"):
        assert rel[k][2::3].tobytes() == hier[k][2::3].tobytes() and np.isfinite(rel[k][2::3]).all()
    assert np.array_equal(rel["n_bad"], hier["n_bad"])


@pytest.mark.parametrize("H, W, T, layout", mr.LINK_SHAPES[:4])
def test_a_linked_row_has_the_bits_of_a_table_that_follows_its_parent_everywhere(libs, device, H, W, T, layout):
    case = mr.links_case(H, W, T, layout)
    rows = case["rows"]
    par = mr.parent_of(rows)[:, 1]
    code, mixed = rt.call(libs["relation"], case, device=device, total=False)
    assert code == 0
    for parent in (0, 2):
        same = rows.copy()
        same[par < 0, 1] = rows[0 if parent == 0 else 1, 1]         # an unlinked row gets a linked record
        same[:, 1]["reserved"] = parent
        assert (mr.parent_of(same)[:, 1] == parent).all()
        code, one = rt.call(libs["relation"], case, device=device, rows=same, total=False)
        assert code == 0
        mine = par == parent
        assert mine.sum() >= 6 and same[mine].tobytes() == rows[mine].tobytes()
        for k in ("ell", "ess"):
            assert mixed[k][mine].tobytes() == one[k][mine].tobytes()


# -- edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, role", mr.EDGE_CASES)
def test_edges_hier(libs, device, kind, role):
    for H in mr.HS8:
        case = mr.chain_case(("edges", kind, role), 257, 1, H)
        got = _chain_against_host(ht, libs["hier"], device, case, ("hier", "edges", kind, role, H), guard=True)
        mr.check_edges_by_hand(kind, role, got)


@pytest.mark.parametrize("kind, role", mr.EDGE_CASES + [(rl.LINGAUSS, "row")])
def test_edges_relation(libs, device, kind, role):
    for H in mr.HS8:
        case = mr.chain_case(("edges", kind, role), 257, 1, H)
        got = _chain_against_host(rt, libs["relation"], device, case, ("relation", "edges", kind, role, H), guard=True)
        mr.check_edges_by_hand(kind, role, got)


@pytest.mark.parametrize("kind, role", mr.EDGE_CASES)
def test_edges_select(libs, device, kind, role):
    for star in range(3):
        case = mr.select_case(("edges", kind, role), 257, T8 + 1, seed=star)
        got = _select_against_host(libs["select"], device, case, ("select", "edges", kind, role, star), guard=True)
        mr.check_edges_by_hand(kind, role, dict(ell=got["ln_alpha"][:, None], ess=got["n_eff"][:, None], n_bad=[got["n_bad"]]))


@pytest.mark.parametrize("kind, role", mr.EDGE_CASES)
def test_edges_reweight(libs, device, kind, role):
    case = mr.reweight_case(("edges", kind, role), 257, 1, T64 + 1)
    got = _reweight_against_host(libs["reweight"], device, case, ("reweight", "edges", kind, role))
    mr.check_edge_weights(kind, role, case, got, rw.want(case))
