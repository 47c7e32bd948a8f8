"""The mixed-row cases of tests/_mixed_rows.py through the four host entries (iso_hier_lnlike_host, iso_select_alpha_host,
iso_reweight_stars_host, iso_relation_lnlike_host), no GPU needed, against the long-double twins within the twins' own
limits; -inf, NaN and n_bad exactly.  And the conditions the device tests rest on, proven on the twins:

* kinds, log_late, log_interim, log_early and links (without the invalid parent): ell, ln_alpha and wsum are finite for every
  (row, star);
* log_*: which (tile, column) computes ln x is what the pattern is for: the last tile only, every tile, the first tile only;
* supports: the dead (row, star) pairs are those of the windows (``dead``, from the construction), every star has a tile
  with a row of full support, a dead row and a row of partial support in that order, and a whole tile without support;
* edges: n_bad, ess of the odd rows and the number of samples without weight are the counts written out by hand in
  tests/_mixed_rows.py for FLAT, POWERLAW and LINGAUSS.

include/isochrones_amd_hier.h on the two records whose bounds are not tested everywhere: LOGNORMAL has "no bounds test"
and CHABRIER tests lo and hi only at and above its break; csrc/common/family_lnf.h and tests/_hier_twin.lnf both do just
that, and the edges cases hold them to it (`test_lognormal_and_chabrier_bounds_are_the_header_s`)."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _hier_cabi as hc, _relation_cabi as rl, _reweight_cabi as rc, _select_cabi as sc
from isochrones_amd.csrc.libraries import HIER, RELATION, REWEIGHT, SELECT
from tests import _hier_twin as ht, _mixed_rows as mr, _relation_twin as rt, _reweight_twin as rw, _select_twin as st

T8, T64, CHUNK = mr.T8, mr.T64, mr.CHUNK


@pytest.fixture(scope="module")
def libs():
    for spec in (HIER, SELECT, REWEIGHT, RELATION):
        spec.build()
    return dict(hier=hc.lib(), select=sc.lib(), reweight=rc.lib(), relation=rl.lib())


# -- the conditions ---------------------------------------------------------------------------------------------------
def check_log_tiles(name, interim, rows, tile):
    need = mr.log_tiles(interim, rows, tile)
    if name == "log_late":
        assert rows.shape[0] % tile != 0 and not need[:-1].any() and need[-1].all()      # the ragged last tile alone
    elif name == "log_early":
        assert need[0].all() and not need[1:].any() and len(need) >= 2
    elif name == "log_interim":
        assert need.all() and not np.isin(rows["kind"], mr.LOG_KINDS).any()
    elif name == "kinds":
        for h0 in range(0, rows.shape[0] - 7):                      # any eight consecutive rows: every kind in every column
            assert all(set(rows[h0:h0 + 8, q]["kind"]) == set(range(1, 9)) for q in range(rows.shape[1]))


def check_supports(x0, rows, dead, tile, neginf=None):
    """``x0`` [S][M]: column 0 by star (or chunk); ``neginf`` [H, S]: where the twin has no support."""
    H, S = dead.shape
    assert neginf is None or np.array_equal(neginf, dead)
    last = ((H - 1) // tile) * tile
    assert dead[last:].all() and last >= tile                       # a whole tile without support, for every star
    for s in range(S):
        inside = mr.support_of_rows(x0[s], rows)
        if x0[s].size > 1:                                          # full, none, partial: the dead row between live ones
            assert inside[0].all() and not inside[1].any() and inside[2].any() and not inside[2].all()
        assert np.array_equal(~inside.any(axis=1), dead[:, s])
    if S > 1:
        assert (dead.any(axis=1) & ~dead.all(axis=1)).any()         # a row dead for one star and alive for its neighbour


def check_chain(name, case, want, tile=T8):
    if name == "supports":
        check_supports(case["x"][0], case["rows"], case["dead"], tile, np.isneginf(want["ell"]))
        assert (want["ess"][case["dead"]] == 0.0).all()
    else:
        check_log_tiles(name, case["interim"], case["rows"], tile)
        assert np.isfinite(want["ell"]).all() and np.isfinite(want["L"]).all()
    assert (want["n_bad"] == 0).all()


# -- the twin of the linked kind dispatches per record ------------------------------------------------------------------
def test_relation_twin_dispatches_per_record():
    case = mr.links_case(2 * T8 + 3, 5, 7)
    rows, x = case["rows"], case["x"]
    par = mr.parent_of(rows)
    assert set(par[:, 1]) == {-1, 0, 2} and set(par[:, 3]) == {-1, 1} and (par[:, [0, 2]] == -1).all()
    assert all(par[h, 1] == (0, 2, -1)[h % 3] for h in range(rows.shape[0]))
    assert {int(k) for k in rows[2::3, 1]["kind"]} == {hc.TRUNCGAUSS, hc.POWERLAW}
    whole = rt.want(case)
    for h in (0, 1, 2, 5, T8, 2 * T8 + 2):
        for q in range(4):
            got = rt.term(rows[h, q], q, x[:, 1])
            want = rt.lingauss(rows[h, q], x[q, 1], x[par[h, q], 1]) if par[h, q] >= 0 else ht.lnf(rows[h, q], x[q, 1])
            assert np.array_equal(got, want)
        alone = rt.lnlike(x, case["interim"], rows[h:h + 1])
        assert np.array_equal(alone["ell"][0], whole["ell"][h]) and np.array_equal(alone["ess"][0], whole["ess"][h])


# -- every pattern through the four host entries ------------------------------------------------------------------------
@pytest.mark.parametrize("name, W, T, H, layout", mr.CHAIN_SHAPES)
def test_hier_host_entry(libs, name, W, T, H, layout):
    case = mr.chain_case(name, W, T, H, layout)
    code, host = ht.call(libs["hier"], case)
    assert code == 0, libs["hier"].iso_hier_last_error()
    ht.assert_matches(host, ht.want(case), (name, W, T, H))
    check_chain(name, case, ht.want(case))


@pytest.mark.parametrize("name, W, T, H, layout", mr.CHAIN_SHAPES)
def test_relation_host_entry(libs, name, W, T, H, layout):
    case = mr.chain_case(name, W, T, H, layout)
    code, host = rt.call(libs["relation"], case)
    assert code == 0, libs["relation"].iso_relation_last_error()
    rt.assert_matches(host, rt.want(case), (name, W, T, H))
    check_chain(name, case, rt.want(case))
    code, hier = ht.call(libs["hier"], case)                        # the same plain loops on the same term: the same bits
    assert code == 0 and all(hier[k].tobytes() == host[k].tobytes() for k in ("ell", "ess", "n_bad", "L", "min_ess"))


@pytest.mark.parametrize("H, W, T, layout", mr.LINK_SHAPES)
@pytest.mark.parametrize("link3", [True, False])
def test_links_host_entry(libs, H, W, T, layout, link3):
    case = mr.links_case(H, W, T, layout, link3)
    par = mr.parent_of(case["rows"])
    assert (par[H - 1, 1] >= 0) == ((H - 1) % 3 != 2)
    assert par[2 * T8 + 2, 1] >= 0 if H == 2 * T8 + 3 else H != 2 * T8 + 2 or par[2 * T8 + 1, 1] < 0    # linked, unlinked last row
    code, host = rt.call(libs["relation"], case)
    assert code == 0, libs["relation"].iso_relation_last_error()
    want = rt.want(case)
    rt.assert_matches(host, want, ("links", H, W, T, link3))
    assert np.isfinite(want["ell"]).all() and np.isfinite(want["L"]).all() and (want["n_bad"] == 0).all()
    # an unlinked POWERLAW row of the linked column makes its tile compute ln x for it
    assert mr.log_tiles(case["interim"], case["rows"], T8)[:, 1].all()


@pytest.mark.parametrize("reserved", [1, 4, -1])                   # itself, past Q, negative: as special_cases()["bad_parent"]
def test_one_invalid_parent_in_the_middle_of_a_tile(libs, reserved):
    H, row = 2 * T8 + 3, T8 + 4
    good, bad = mr.links_case(H, 5, 7), mr.links_case(H, 5, 7, bad=(row, reserved))
    code, host = rt.call(libs["relation"], bad)
    assert code == 0, libs["relation"].iso_relation_last_error()
    rt.assert_matches(host, rt.want(bad), ("bad parent", reserved))
    code, ref = rt.call(libs["relation"], good)
    assert code == 0
    others = np.arange(H) != row
    assert np.isneginf(host["ell"][row]).all() and (host["ess"][row] == 0.0).all() and list(host["n_bad"]) == [0, 0, 0]
    assert np.isneginf(host["L"][row]) and host["min_ess"][row] == 0.0
    for k in ("ell", "ess", "L", "min_ess"):
        assert host[k][others].tobytes() == ref[k][others].tobytes() and np.isfinite(host[k][others]).all()


@pytest.mark.parametrize("name, J, H", mr.SELECT_SHAPES)
def test_select_host_entry(libs, name, J, H):
    case = mr.select_case(name, J, H)
    code, host = st.call(libs["select"], case)
    assert code == 0, libs["select"].iso_select_last_error()
    want = st.want(case)
    st.assert_matches(host, want, (name, J, H))
    assert want["n_bad"] == 0
    if name == "supports":
        nchunks = -(-J // CHUNK)
        x0 = [case["x"][0, c * CHUNK:(c + 1) * CHUNK] for c in range(nchunks)]
        check_supports(x0, case["rows"], case["dead"], T8)
        assert np.array_equal(np.isneginf(want["ln_alpha"]), case["dead"].all(axis=1))
        if nchunks == 2:                                            # rows with support in the one chunk only, either way round
            assert (case["dead"][:, 0] & ~case["dead"][:, 1]).any() and (~case["dead"][:, 0] & case["dead"][:, 1]).any()
    else:
        check_log_tiles(name, case["draw"], case["rows"], T8)
        assert np.isfinite(want["ln_alpha"]).all()


@pytest.mark.parametrize("name, W, T, H, layout", mr.REWEIGHT_SHAPES)
def test_reweight_host_entry(libs, name, W, T, H, layout):
    case = mr.reweight_case(name, W, T, H, layout)
    code, host = rw.call(libs["reweight"], case)
    assert code == 0, libs["reweight"].iso_reweight_last_error()
    want = rw.want(case)
    rw.assert_matches(host, want, (name, W, T, H))                  # no near tie in the case: asserted there
    assert (want["n_bad"] == 0).all() and np.isfinite(want["wsum"]).all() and (want["wsum"] > 0).all()
    ell = rw.ell(case)
    if name == "supports":
        check_supports(case["x"][0], case["rows"], case["dead"], T64, np.isneginf(ell))
    else:
        check_log_tiles(name, case["interim"], case["rows"], T64)
        assert np.isfinite(ell).all()


# -- edges --------------------------------------------------------------------------------------------------------------
def test_the_edge_values_are_where_a_kernel_can_lose_them():
    for kind, role in mr.EDGE_CASES:
        rec = ht.all_kinds()[kind]
        vals = mr.edge_values(rec)
        x = mr.chain_case(("edges", kind, role), 257, 1, T8 + 1)["x"][0]
        for at in (0, 63, 64, 255, 256):
            seen = x[:, at]
            assert all(any(v.tobytes() == e.tobytes() for e in vals) for v in seen), (kind, at)
        met = {v.tobytes() for v in x[:, [0, 63, 64, 255, 256]].ravel()}
        assert met == {e.tobytes() for e in vals}                   # every value at one of the five places in some star
        assert (len(vals) == 13) == (kind == hc.CHABRIER)


@pytest.mark.parametrize("kind, role", mr.EDGE_CASES)
@pytest.mark.parametrize("H", mr.HS8)
def test_edges_hier_and_relation_host_entries(libs, kind, role, H):
    case = mr.chain_case(("edges", kind, role), 257, 1, H)
    code, host = ht.call(libs["hier"], case)
    assert code == 0, libs["hier"].iso_hier_last_error()
    ht.assert_matches(host, ht.want(case), ("edges", kind, role))
    mr.check_edges_by_hand(kind, role, host)
    code, rel = rt.call(libs["relation"], case)
    assert code == 0 and all(rel[k].tobytes() == host[k].tobytes() for k in ("ell", "ess", "n_bad", "L", "min_ess"))


@pytest.mark.parametrize("H", mr.HS8)
def test_edges_of_the_linked_kind_host_entry(libs, H):
    case = mr.chain_case(("edges", rl.LINGAUSS, "row"), 257, 1, H)
    code, host = rt.call(libs["relation"], case)
    assert code == 0, libs["relation"].iso_relation_last_error()
    rt.assert_matches(host, rt.want(case), ("edges", "lingauss"))
    mr.check_edges_by_hand(rl.LINGAUSS, "row", host)


@pytest.mark.parametrize("kind, role", mr.EDGE_CASES)
def test_edges_select_host_entry(libs, kind, role):
    for star in range(3):
        case = mr.select_case(("edges", kind, role), 257, T8 + 1, seed=star)
        code, host = st.call(libs["select"], case)
        assert code == 0, libs["select"].iso_select_last_error()
        st.assert_matches(host, st.want(case), ("edges", kind, role, star))
        mr.check_edges_by_hand(kind, role, dict(ell=host["ln_alpha"][:, None], ess=host["n_eff"][:, None], n_bad=[host["n_bad"]]))


@pytest.mark.parametrize("kind, role", mr.EDGE_CASES)
def test_edges_reweight_host_entry(libs, kind, role):
    case = mr.reweight_case(("edges", kind, role), 257, 1, T64 + 1)
    code, host = rw.call(libs["reweight"], case)
    assert code == 0, libs["reweight"].iso_reweight_last_error()
    rw.assert_matches(host, rw.want(case), ("edges", kind, role))
    mr.check_edge_weights(kind, role, case, host, rw.want(case))


def test_lognormal_and_chabrier_bounds_are_the_header_s(libs):
    """LOGNORMAL: no bounds test, so a value outside [lo, hi] has a density unless ln x fails; CHABRIER: below the break lo
    is not tested (0.05 < lo = 0.1 has the log-normal branch's density), at and above it lo and hi are."""
    kinds = ht.all_kinds()
    rec = np.concatenate([kinds[hc.LOGNORMAL], kinds[hc.CHABRIER]])
    rec[0]["lo"], rec[0]["hi"] = 0.5, 2.0                           # bounds a LOGNORMAL record ignores
    rec[1]["lo"] = 0.1                                              # below the break: a bound the record does not test there
    brk, hi_ = float(rec[1]["p"][5]), float(rec[1]["hi"])
    assert brk > 0.1
    x = np.array([0.25, 4.0, 0.0, -0.0, -1.0, np.inf, 0.05, 5e-324, np.nextafter(brk, 0.0), brk, hi_, np.nextafter(hi_, np.inf)])
    out = np.full((2, x.size), -7.0)
    assert libs["hier"].iso_hier_lnpdf_host(C.c_void_p(rec.ctypes.data), 2, C.c_void_p(x.ctypes.data), x.size,
                                            C.c_void_p(out.ctypes.data)) == 0
    twin = np.stack([ht.lnf(rec[i], x) for i in range(2)]).astype(np.float64)
    assert np.array_equal(np.isnan(out), np.isnan(twin)) and np.array_equal(np.isneginf(out), np.isneginf(twin))
    fin = np.isfinite(twin)
    assert np.all(np.abs(out[fin] - twin[fin]) <= 1e-12 * np.maximum(1.0, np.abs(twin[fin])))
    assert np.isfinite(out[0, [0, 1, 7]]).all() and np.isnan(out[0, 2:5]).all() and np.isneginf(out[0, 5])
    assert np.isfinite(out[1, [6, 7, 8, 9, 10]]).all() and np.isnan(out[1, 2:5]).all() and np.isneginf(out[1, [5, 11]]).all()
