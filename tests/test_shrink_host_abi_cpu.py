"""libiso_shrink.so's host entries through ctypes, no GPU needed: iso_shrink_cells_host and iso_shrink_weights_host against
the long-double twin of tests/_shrink_twin.py within 1e-11 relative, wsum = live rows x M, the restated per-sample term
held to binned.hip's bit for bit, the identity with iso_reweight_stars_host on a flat population, the edge cases of the
bins, the rows and the cells, every refusal with its message."""
import numpy as np
import pytest

from isochrones_amd import _binned_cabi as bc, _reweight_cabi as rc, _shrink_cabi as sc, hierarchical as hi
from isochrones_amd import priors as P
from isochrones_amd.csrc.libraries import BINNED, HIER, REWEIGHT, SHRINK
from tests import _binned_twin as bt, _hier_twin as tw, _reweight_twin as rt, _shrink_twin as st

PM, RM = bt.PM, bt.RM


@pytest.fixture(scope="module")
def libs():
    for spec in (HIER, BINNED, REWEIGHT, SHRINK):
        spec.build()
    return bc.lib(), sc.lib()


def _err(lib):
    return lib.iso_shrink_last_error().decode()


@pytest.mark.parametrize("S, W, T, n_bins, H, layout, n_frozen", [
    (3, 5, 7, (4,), 3, PM, 1), (2, 16, 16, (1,), 1, RM, 0), (3, 7, 11, (64,), 9, PM, 2), (3, 5, 7, (3, 5), 8, RM, 1),
    (2, 8, 9, (8, 8), 17, PM, 2), (2, 4, 5, (2, 1), 2, PM, 0)])
def test_host_entries_match_the_twin(libs, S, W, T, n_bins, H, layout, n_frozen):
    blib, lib = libs
    case = bt.make_case(S, W, T, n_bins, H, seed=3 + H + W, layout=layout, n_frozen=n_frozen)
    tab, out, cel, wts = st.run(blib, lib, case)
    lnG, cellp = st.cells(tab["A"], tab["mx"], case["lnh"], out["ell"])
    worst = [st.close(cel["lnG"], lnG, log=True), st.close(cel["cellp"], cellp)]
    want = st.weights(case, tab["mx"], cel["lnG"])
    worst += [st.close(wts["weights"], want["u"]), st.close(wts["wsum"], want["wsum"]), st.close(wts["ess"], want["ess"])]
    print("against the twin: worst error / limit = %.3f" % max(worst))
    assert np.array_equal(wts["n_bad"], want["n_bad"]) and np.array_equal(wts["n_out"], want["n_out"])
    assert np.array_equal(wts["n_bad"], tab["n_bad"]) and np.array_equal(wts["n_out"], tab["n_out"]) and (tab["n_out"] > 0).any()
    # with ell the likelihood's own normaliser a star's weights sum to M per live row, its cell probabilities to 1
    live = np.isfinite(out["ell"]).sum(axis=0)
    assert (live > 0).all() and np.all(np.abs(wts["wsum"] - live * (W * T)) <= 1e-11 * live * (W * T))
    assert np.all(np.abs(cel["cellp"].sum(axis=0) - 1.0) <= 1e-11) and np.all(cel["cellp"] >= 0)
    # the cell probabilities are the weights summed per cell
    _, cell, _, _ = bt.sample_terms(case)
    for s in range(S):
        per_cell = np.bincount(cell[s][cell[s] >= 0], wts["weights"][s][cell[s] >= 0], minlength=cel["cellp"].shape[0])
        assert np.allclose(per_cell / wts["wsum"][s], cel["cellp"][:, s], rtol=0, atol=1e-11)
    # without cellp the same lnG
    code, again = st.call_cells(lib, tab, case["lnh"], out["ell"], with_p=False)
    assert code == 0 and again["lnG"].tobytes() == cel["lnG"].tobytes() and (again["cellp"] == -7.0).all()


@pytest.mark.parametrize("n_bins, layout, n_frozen", [((5,), PM, 1), ((3, 4), RM, 2), ((1,), PM, 0), ((64,), RM, 1)])
def test_the_two_copies_of_the_sample_term_agree_bit_for_bit(libs, n_bins, layout, n_frozen):
    """H = 1, lnh = 0 and ell = mx make every a_h = 0, so lnG = 0 and u = exp(c_m - mx): the weights of
    common/binned_sample.h summed per cell in ascending m are A of binned.hip's own sample_term, and the counts are its
    counts."""
    blib, lib = libs
    S, W, T = 4, 7, 19
    case = bt.make_case(S, W, T, n_bins, 1, seed=11 + len(n_bins), layout=layout, n_frozen=n_frozen)
    x = case["x"].copy()
    x[case["axes"][0], 0, 5] = np.nan                                # a bad sample
    x[case["axes"][0], 1, :] = 99.0                                  # a star with every sample out of the interim prior
    case = bt.replace_x(case, x)
    code, tab = bt.call_compress(blib, case)
    assert code == 0
    B = bt.n_cells(case)
    code, cel = st.call_cells(lib, tab, np.zeros((1, B)), tab["mx"][None, :])
    assert code == 0, _err(lib)
    filled = np.isfinite(tab["mx"])
    assert filled.sum() == S - 1 and (cel["lnG"][:, filled] == 0.0).all() and np.isneginf(cel["lnG"][:, ~filled]).all()
    code, wts = st.call_weights(lib, case, tab["mx"], cel["lnG"])
    assert code == 0, _err(lib)
    _, cell, _, _ = bt.sample_terms(case)
    A = np.zeros((B, S))
    for s in range(S):
        for m in range(W * T):                                       # ascending m, each sum from 0.0
            if cell[s, m] >= 0:
                A[cell[s, m], s] += wts["weights"][s, m]
        assert (wts["weights"][s][cell[s] < 0] == 0.0).all()
    assert A.tobytes() == tab["A"].tobytes()
    assert np.array_equal(wts["n_bad"], tab["n_bad"]) and np.array_equal(wts["n_out"], tab["n_out"])


@pytest.mark.parametrize("n_axes, layout", [(1, PM), (2, RM)])
def test_a_uniform_histogram_is_a_flat_population(libs, n_axes, layout):
    """Equal heights over the full interim range: the weights (normalised by wsum), ess and the summaries are
    iso_reweight_stars_host's on Fixed(FlatPrior(range)) columns."""
    blib, lib = libs
    rlib = rc.lib()
    rng = np.random.default_rng(n_axes)
    S, W, T = 3, 5, 31
    M = W * T
    ranges = [(8.0, 10.0), (-1.0, 0.5)][:n_axes]
    x = np.stack([rng.uniform(lo - 0.05, hi_ + 0.05, (S, M)) for lo, hi_ in ranges] + [rng.uniform(0.3, 2.5, (S, M))])
    interim_p = [P.GaussianPrior(0.5 * (lo + hi_), 0.8) for lo, hi_ in ranges] + [P.FlatPrior((0.1, 10.0))]
    frozen_p = P.PowerLawPrior(-2.35, (0.1, 10.0))
    Q = n_axes + 1
    interim = np.concatenate([hi.prior_record(p) for p in interim_p])
    frozen = hi.records(Q)
    frozen[Q - 1] = hi.prior_record(frozen_p)[0]
    edges = [np.linspace(lo, hi_, k + 1) for (lo, hi_), k in zip(ranges, (6, 3))]
    B = int(np.prod([len(e) - 1 for e in edges]))
    lnh = np.full((1, B), -np.sum([np.log(hi_ - lo) for lo, hi_ in ranges]))
    case = dict(x=x, interim=interim, frozen=frozen, frozen_cols=(Q - 1,), axes=tuple(range(n_axes)), edges=edges, S=S, W=W, T=T,
                layout=layout, mask=None, extra=None, lnh=lnh)
    case["storages"], case["where"] = tw.place(x, W, T, layout, 0)
    tab, out, cel, wts = st.run(blib, lib, case)
    assert (tab["n_out"] > 0).all()
    probs = (0.16, 0.5, 0.84)
    code, got = st.call_summary(rlib, case, list(range(Q)), wts["weights"], probs)
    assert code == 0
    # the same columns as a reweighting case: the population is flat on the grid's range, the frozen column's record
    flat = rt.fixed_case(x, x, interim_p, [[P.FlatPrior(r) for r in ranges] + [frozen_p]], W, T, probs=probs, layout=layout)
    flat["values"] = [("x", q) for q in range(Q)]
    code, ref = rt.call(rlib, flat)
    assert code == 0 and (ref["n_bad"] == 0).all()
    assert np.array_equal(ref["weights"] == 0, wts["weights"] == 0) and (wts["weights"] == 0).sum() == tab["n_out"].sum()
    st.close(wts["weights"] / wts["wsum"][:, None], ref["weights"] / ref["wsum"][:, None])
    st.close(wts["ess"], ref["ess"])
    st.close(got["mean"], ref["mean"], log=True)
    st.close(got["sd"], ref["sd"])
    assert np.array_equal(got["quant"], ref["quant"]) and np.array_equal(got["n_nan"], ref["n_nan"])


def test_the_last_edge_and_samples_outside(libs):
    blib, lib = libs
    edges = np.array([0.0, 0.5, 2.0, 2.25, 4.0])
    below, above = np.nextafter(0.0, -1.0), np.nextafter(4.0, 5.0)
    x = np.array([[0.0, 0.5, np.nextafter(0.5, 0.0), 2.0, 2.25, 4.0, np.nextafter(4.0, 0.0), below, above, -3.0, 1.0, np.nan],
                  [5.0, 6.0, 7.0, 8.0, -1.0, -2.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0]])
    lnh = np.log([[0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, 0.1]])
    case = bt.one_axis_case(x, edges, W=3, T=4, lnh=lnh)
    tab, out, cel, wts = st.run(blib, lib, case)
    w = wts["weights"]
    # x == e[K] is in the last bin, a step beyond it is out, and so is a step below e[0]; the NaN is bad
    assert (w[0, :7] > 0).all() and (w[0, 7:10] == 0).all() and w[0, 10] > 0 and w[0, 11] == 0
    assert w[0, 4] == w[0, 5] == w[0, 6] and w[0, 0] == w[0, 2] and w[0, 1] != w[0, 0]
    assert wts["n_out"].tolist() == [3, 12] and wts["n_bad"].tolist() == [1, 0]
    # a flat interim prior: a sample's weight is its cell's G alone
    G = np.exp(cel["lnG"][:, 0])
    assert np.allclose(w[0, [0, 1, 2, 3, 4, 5, 6, 10]], G[[0, 1, 0, 2, 3, 3, 3, 1]], rtol=1e-14, atol=0)
    # the star with every sample out: no weight, no effective sample, NaN summaries, NaN cell probabilities
    assert wts["wsum"][1] == 0.0 and wts["ess"][1] == 0.0 and (w[1] == 0).all()
    assert np.isneginf(cel["lnG"][:, 1]).all() and np.isnan(cel["cellp"][:, 1]).all()
    code, got = st.call_summary(rc.lib(), case, [0], w, (0.5,))
    assert code == 0 and np.isnan(got["mean"][1, 0]) and np.isnan(got["sd"][1, 0]) and np.isnan(got["quant"][1, 0, 0])
    assert got["n_nan"][:, 0].tolist() == [1, 0] and np.isfinite(got["mean"][0, 0])
    st.close(wts["weights"], st.weights(case, tab["mx"], cel["lnG"])["u"])


def test_masked_stars_dead_rows_and_empty_cells(libs):
    blib, lib = libs
    rng = np.random.default_rng(2)
    x = rng.uniform(0.0, 3.0, (3, 35))
    x[1] = rng.uniform(0.0, 1.0, 35)                                 # star 1 lies in bin 0 alone
    lnh = np.array([[0.0, -np.inf, 0.3], [-np.inf, 0.2, 0.1], [-np.inf, -np.inf, -np.inf], [np.nan, 0.0, np.nan], [0.2, 0.1, 0.0]])
    case = bt.one_axis_case(x, [0.0, 1.0, 2.0, 3.0], W=5, T=7, lnh=lnh, mask=[1, 1, 0])
    tab, out, cel, wts = st.run(blib, lib, case)
    # star 1: rows 1, 2 and 3 have ell = -inf (no height where it lies); star 0: row 2 alone
    assert np.isneginf(out["ell"][[1, 2, 3], 1]).all() and np.isneginf(out["ell"][2, 0]) and np.isfinite(out["ell"][[0, 1, 3, 4], 0]).all()
    lnG, cellp = st.cells(tab["A"], tab["mx"], lnh, out["ell"], case["mask"])
    st.close(cel["lnG"], lnG, log=True)
    st.close(cel["cellp"], cellp)
    assert np.isfinite(cel["lnG"][:, 0]).all() and np.isfinite(cel["lnG"][0, 1])
    assert cel["cellp"][:, 1].tolist() == [1.0, 0.0, 0.0]             # no sample of star 1 in the other cells
    assert np.abs(wts["wsum"][:2] - np.array([4, 2]) * 35.0).max() <= 1e-11 * 4 * 35
    # the masked star: NaN, counts 0, its weights not written
    assert np.isnan(cel["lnG"][:, 2]).all() and np.isnan(cel["cellp"][:, 2]).all()
    assert np.isnan(wts["wsum"][2]) and np.isnan(wts["ess"][2]) and wts["n_bad"][2] == 0 and wts["n_out"][2] == 0
    assert (wts["weights"][2] == -7.0).all() and (wts["weights"][:2] >= 0).all()
    # a cell whose every height is 0: lnG = -inf there, its samples weigh nothing
    dead = lnh.copy()
    dead[:, 1] = -np.inf
    dcase = dict({k: v for k, v in case.items() if k != "want"}, lnh=dead)
    dtab, dout, dcel, dwts = st.run(blib, lib, dcase)
    assert np.isneginf(dcel["lnG"][1, :2]).all() and (dcel["cellp"][1, :2] == 0).all()
    _, cell, _, _ = bt.sample_terms(dcase)
    assert (dwts["weights"][0][cell[0] == 1] == 0).all() and (dwts["weights"][0][cell[0] == 0] > 0).all()
    st.close(dwts["weights"][:2], st.weights(dcase, dtab["mx"], dcel["lnG"])["u"][:2])
    # a sub-range writes its stars and leaves the rest alone
    code, part = st.call_cells(lib, tab, lnh, out["ell"], case["mask"], ens_begin=1, n_ens_out=1)
    assert code == 0 and (part["lnG"][:, [0, 2]] == -7.0).all() and (part["cellp"][:, [0, 2]] == -7.0).all()
    assert part["lnG"][:, 1].tobytes() == cel["lnG"][:, 1].tobytes() and part["cellp"][:, 1].tobytes() == cel["cellp"][:, 1].tobytes()
    code, pw = st.call_weights(lib, case, tab["mx"], cel["lnG"], ens_begin=1, n_ens_out=1)
    assert code == 0 and (pw["wsum"][[0, 2]] == -7.0).all() and (pw["n_out"][[0, 2]] == -7).all()
    assert pw["weights"][0].tobytes() == wts["weights"][1].tobytes() and pw["wsum"][1] == wts["wsum"][1]


def test_a_first_offset_and_the_other_layout(libs):
    blib, lib = libs
    case = bt.make_case(4, 5, 7, (3, 2), 3, seed=6, layout=PM, n_frozen=1)
    tab, out, cel, wts = st.run(blib, lib, case)
    other = bt.replace_x(case, case["x"], layout=RM)
    code, got = st.call_weights(lib, other, tab["mx"], cel["lnG"])
    assert code == 0
    for k in ("weights", "wsum", "ess", "n_bad", "n_out"):
        assert got[k].tobytes() == wts[k].tobytes(), k
    # the stars 2 and 3 from storages that hold only them (first = 2)
    S, W, T = case["S"], case["W"], case["T"]
    sub, where = tw.place(case["x"][:, 2:4], W, T, PM, 5)
    cols = [(k, nc, col, 2, 2) for k, nc, col in where]
    code, got = st.call_weights(lib, case, tab["mx"], cel["lnG"], ens_begin=2, n_ens_out=2, cols=cols, storages=sub)
    assert code == 0, _err(lib)
    assert got["weights"].tobytes() == wts["weights"][2:4].tobytes() and got["wsum"][2:].tobytes() == wts["wsum"][2:].tobytes()
    assert got["ess"][2:].tobytes() == wts["ess"][2:].tobytes() and np.array_equal(got["n_out"][2:], wts["n_out"][2:])


REFUSALS = [
    (dict(n_bins=[65]), "more than 64 cells"), (dict(n_bins=[9, 8], n_axes=2, axis_col=[0, 1], n_frozen=0), "more than 64 cells"),
    (dict(n_axes=3, axis_col=[0, 1, 1], n_bins=[2, 2, 2]), "1 or 2 binned axes"), (dict(n_axes=0), "1 or 2 binned axes"),
    (dict(frozen_col=[0, 1], n_frozen=2), "both as a binned axis and as frozen"),
    (dict(frozen_col=[], n_frozen=0), "neither a binned axis nor frozen"),
    (dict(axis_col=[0, 0], n_axes=2, n_bins=[2, 2]), "binned axis twice"), (dict(axis_col=[2]), "no column"),
    (dict(n_bins=[0]), "at least 1 bin"),
    (dict(Q=0), "Q must be 1 to 4"), (dict(Q=5), "Q must be 1 to 4"), (dict(layout=7), "unknown chain layout"),
    (dict(T=0), "at least 1"), (dict(T=(2 ** 31 - 1) // 3), "2^31 - 257 samples"),
    (dict(edges=[0.0, 1.0, 1.0, 2.0, 3.0]), "finite and strictly increasing"),
    (dict(edges=[0.0, np.nan, 2.0, 3.0, 4.0]), "finite and strictly increasing"),
]


@pytest.mark.parametrize("over, message", REFUSALS)
def test_refusals(libs, over, message):
    blib, lib = libs
    case = bt.make_case(2, 3, 4, (4,), 1, seed=1, n_frozen=1)          # Q = 2: column 0 binned, column 1 frozen
    tab, out, cel, wts = st.run(blib, lib, case)
    code, got = st.call_weights(lib, case, tab["mx"], cel["lnG"], **over)
    assert code == sc.ERR_INVALID and message in _err(lib), _err(lib)
    assert _err(lib).startswith("iso_shrink_weights_host: ") and (got["weights"] == -7.0).all() and (got["wsum"] == -7.0).all()


def test_refused_ranges_records_and_cells(libs):
    blib, lib = libs
    case = bt.make_case(2, 3, 4, (4,), 1, seed=1, n_frozen=1)
    tab, out, cel, wts = st.run(blib, lib, case)
    for kw in (dict(ens_begin=2, n_ens_out=1), dict(ens_begin=0, n_ens_out=0), dict(ens_begin=1, n_ens_out=2)):
        assert st.call_weights(lib, case, tab["mx"], cel["lnG"], **kw)[0] == sc.ERR_INVALID and "ensemble range" in _err(lib)
    cols = [(k, nc, col, 1, 1) for k, nc, col in case["where"]]
    assert st.call_weights(lib, case, tab["mx"], cel["lnG"], cols=cols)[0] == sc.ERR_INVALID
    assert "does not hold the ensembles" in _err(lib)
    bad = dict(case, frozen=case["frozen"].copy())
    bad["frozen"]["kind"][1] = 9
    assert st.call_weights(lib, bad, tab["mx"], cel["lnG"])[0] == sc.ERR_INVALID and "kinds 1 to 8" in _err(lib)
    for kw, message in ((dict(B=65), "1 to 64 cells"), (dict(B=0), "1 to 64 cells"), (dict(ens_begin=2), "ensemble range")):
        assert st.call_cells(lib, tab, case["lnh"], out["ell"], **kw)[0] == sc.ERR_INVALID and message in _err(lib)
        assert _err(lib).startswith("iso_shrink_cells_host: ")
    assert st.call_cells(lib, tab, case["lnh"][:0], out["ell"][:0])[0] == sc.ERR_INVALID and "H must be" in _err(lib)
    inf = case["lnh"].copy()
    inf[0, 2] = np.inf
    code, got = st.call_cells(lib, tab, inf, out["ell"])
    assert code == sc.ERR_INVALID and "+inf" in _err(lib) and (got["lnG"] == -7.0).all()
    import ctypes as C
    a = C.c_void_p(tab["A"].ctypes.data)
    assert lib.iso_shrink_cells_host(a, a, 4, 2, 0, 2, a, a, 1, None, None, None, None) == sc.ERR_INVALID
    assert "null pointer" in _err(lib)
