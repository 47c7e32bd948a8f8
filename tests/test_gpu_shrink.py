"""iso_shrink_cells and iso_shrink_weights (k_shrink_cells, k_shrink_weights) with iso_reweight_summary on the device against
the host entries: S = 1, 3 (the middle star masked) and 257 (a second block of stars); M = 1, 256 (exactly one sample a
lane), 265 (a tail of 9) and 259; B = 1, 5 and 8 x 8 (one cell, a ragged last tile of cells, 32 tiles); H = 1, 9 and 65;
both layouts; edge, out, bad and NaN samples in lane 0, lane 255 and the tail.  Bit identity: a star alone, in the batch and
in a sub-range, from the other layout, from a copied column with a `first` offset, on a second call; a (star, cell) in
another block of stars and in another tile of cells (the rows are not tiled: a lane walks all H of them)."""
import numpy as np
import pytest

from isochrones_amd import _binned_cabi as bc, _reweight_cabi as rc, _shrink_cabi as sc
from tests import _binned_twin as bt, _hier_twin as tw, _reweight_twin as rt, _shrink_twin as st

pytestmark = pytest.mark.gpu
PM, RM = bt.PM, bt.RM
PROBS = (0.16, 0.5, 0.84)


@pytest.fixture(scope="module")
def libs():
    return bc.lib(), sc.lib(), rc.lib()


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _special(case):
    """The case with an edge, an out, a bad and a NaN sample in lane 0, lane 255 and the tail of the first and last star."""
    x = case["x"].copy()
    M = x.shape[2]
    a0 = case["axes"][0]
    e = case["edges"][0]
    spots = sorted({0, min(255, M - 1), M - 1})
    values = [e[0], e[-1], e[len(e) // 2], np.nextafter(e[-1], 99.0), np.nan]
    for i, m in enumerate(spots):
        x[a0, 0, m] = values[i % 5]
        x[a0, -1, m] = values[(i + 3) % 5]
    if M > 4:
        x[a0, 0, 1:4] = e[-1], np.nextafter(e[0], -99.0), np.nan
    return bt.replace_x(case, x)


def _mask(S):
    if S == 1:
        return None
    mask = np.ones(S, np.int32)
    mask[1] = 0
    return mask


#        S,  W,  T,  n_bins, H, layout
SHAPES = [(1, 1, 1, (1,), 1, PM), (3, 32, 8, (5,), 9, RM), (3, 5, 53, (8, 8), 65, PM), (3, 7, 37, (1,), 65, RM),
          (257, 32, 8, (5,), 9, PM), (3, 7, 37, (8, 8), 1, RM), (1, 5, 53, (5,), 65, PM), (257, 1, 1, (8, 8), 9, RM)]


@pytest.mark.parametrize("S, W, T, n_bins, H, layout", SHAPES)
def test_device_matches_the_host_entries(libs, device, S, W, T, n_bins, H, layout):
    blib, lib, rlib = libs
    n_frozen = 1
    case = _special(bt.make_case(S, W, T, n_bins, H, seed=S + W + H, layout=layout, n_frozen=n_frozen, mask=_mask(S)))
    what = (S, W, T, n_bins, H, layout)
    htab, hout, hcel, hwts = st.run(blib, lib, case)
    dtab, dout, dcel, dwts = st.run(blib, lib, case, device=device)
    worst = [st.close(dcel["lnG"], hcel["lnG"], log=True), st.close(dcel["cellp"], hcel["cellp"]),
             st.close(dwts["weights"], hwts["weights"]), st.close(dwts["wsum"], hwts["wsum"]), st.close(dwts["ess"], hwts["ess"])]
    print(what, "device against host: worst error / limit = %.3f" % max(worst))
    assert np.array_equal(dwts["n_bad"], hwts["n_bad"]) and np.array_equal(dwts["n_out"], hwts["n_out"]), what
    live = np.isfinite(dout["ell"]).sum(axis=0).astype(np.float64)
    keep = np.ones(S, bool) if case["mask"] is None else case["mask"] != 0
    assert np.all(np.abs(dwts["wsum"][keep] - live[keep] * (W * T)) <= 1e-11 * np.maximum(live[keep], 1) * (W * T)), what
    has = keep & (dwts["wsum"] > 0)
    assert np.all(np.abs(dcel["cellp"][:, has].sum(axis=0) - 1.0) <= 1e-11), what
    if S > 1:
        assert np.isnan(dcel["lnG"][:, 1]).all() and np.isnan(dwts["wsum"][1]) and (dwts["weights"][1] == -7.0).all()
    # the summaries of every column under the device's weights, against the host entry under the host's
    Q = case["x"].shape[0]
    code, hsum = st.call_summary(rlib, case, list(range(Q)), hwts["weights"], PROBS)
    assert code == 0
    code, dsum = st.call_summary(rlib, case, list(range(Q)), dwts["weights"], PROBS, device=device)
    assert code == 0, rlib.iso_reweight_last_error()
    assert np.array_equal(dsum["n_nan"], hsum["n_nan"]), what
    st.close(dsum["sd"], hsum["sd"])
    scale = np.nanmax(np.abs(case["x"]), axis=2).T                  # [S, Q]
    fin = np.isfinite(hsum["mean"])
    assert np.array_equal(np.isnan(dsum["mean"]), np.isnan(hsum["mean"])), what
    assert np.all(np.abs(dsum["mean"] - hsum["mean"])[fin] <= 1e-11 * scale[fin]), what
    # quantiles as tests/test_gpu_reweight.py compares them: equal, unless some cumulated weight lies within rounding of a target
    near = np.zeros(hsum["quant"].shape, bool)
    for s in np.flatnonzero(keep):
        for q in range(Q):
            near[s, q] = rt.summary(hwts["weights"][s].astype(np.longdouble), case["x"][q, s], PROBS)[4]
    assert not near.any(), (what, "the case has a near tie: pick another seed")
    assert np.array_equal(dsum["quant"], hsum["quant"], equal_nan=True), what


def _same(a, b, keys):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)


@pytest.mark.parametrize("W, T, n_bins", [(32, 8, (5,)), (5, 53, (8, 8)), (7, 37, (1,))])
def test_a_stars_weights_are_bit_identical(libs, device, W, T, n_bins):
    blib, lib, _ = libs
    S = 4
    case = _special(bt.make_case(S, W, T, n_bins, 9, seed=5, layout=PM, n_frozen=1))
    tab, out, cel, full = st.run(blib, lib, case, device=device)
    mx, lnG = tab["mx"], cel["lnG"]
    keys = ("weights", "wsum", "ess", "n_bad", "n_out")
    code, again = st.call_weights(lib, case, mx, lnG, device=device)                       # a second call
    assert code == 0 and _same(again, full, keys)
    other = dict(case, layout=RM)
    other["storages"], other["where"] = tw.place(case["x"], W, T, RM, 3)
    code, got = st.call_weights(lib, other, mx, lnG, device=device)                        # the other layout, other storages
    assert code == 0 and _same(got, full, keys)
    for s in range(S):                                                                     # a star alone
        alone = bt.replace_x(case, case["x"][:, s:s + 1], S=1)
        code, got = st.call_weights(lib, alone, mx[s:s + 1], lnG[:, s:s + 1], device=device)
        assert code == 0 and got["weights"][0].tobytes() == full["weights"][s].tobytes(), s
        assert all(got[k][0].tobytes() == full[k][s].tobytes() for k in keys[1:]), s
    code, part = st.call_weights(lib, case, mx, lnG, device=device, ens_begin=1, n_ens_out=2)      # a sub-range
    assert code == 0 and part["weights"].tobytes() == full["weights"][1:3].tobytes()
    assert all(part[k][1:3].tobytes() == full[k][1:3].tobytes() for k in keys[1:])
    assert (part["wsum"][[0, 3]] == -7.0).all() and (part["n_out"][[0, 3]] == -7).all()
    # a derived-style second storage: the binned axis of the stars [1, 3) alone in a storage of its own, first = 1
    sub, where = tw.place(case["x"][:, 1:3], W, T, PM, 8)
    n0 = len(case["storages"])
    axis = case["axes"][0]
    cols = [(n0 + k, nc, col, 2, 1) if q == axis else (case["where"][q] + (S, 0)) for q, (k, nc, col) in enumerate(where)]
    code, moved = st.call_weights(lib, case, mx, lnG, device=device, ens_begin=1, n_ens_out=2, cols=cols,
                                  storages=case["storages"] + sub)
    assert code == 0 and moved["weights"].tobytes() == full["weights"][1:3].tobytes()
    assert all(moved[k][1:3].tobytes() == full[k][1:3].tobytes() for k in keys[1:])


def test_a_cell_is_bit_identical_in_any_block_and_tile(libs, device):
    blib, lib, _ = libs
    S, H = 257, 65
    mask = np.ones(S, np.int32)
    mask[3] = 0
    case = bt.make_case(S, 5, 7, (8, 8), H, seed=11, mask=mask)
    tab, out = bt.run(blib, case, device=device)
    code, full = st.call_cells(lib, tab, case["lnh"], out["ell"], mask, device=device)
    assert code == 0 and np.isfinite(full["lnG"][:, 256]).any() and np.isnan(full["lnG"][:, 3]).all()
    code, again = st.call_cells(lib, tab, case["lnh"], out["ell"], mask, device=device)    # a second call
    assert code == 0 and _same(again, full, ("lnG", "cellp"))
    # the last star (lane 0 of the second block) alone: lane 0 of the first block
    one = dict(A=np.ascontiguousarray(tab["A"][:, 256:]), mx=tab["mx"][256:])
    code, alone = st.call_cells(lib, one, case["lnh"], np.ascontiguousarray(out["ell"][:, 256:]), device=device)
    assert code == 0 and alone["lnG"][:, 0].tobytes() == full["lnG"][:, 256].tobytes()
    assert alone["cellp"][:, 0].tobytes() == full["cellp"][:, 256].tobytes()
    # sub-ranges of the stars write their own and leave the rest: the star at lane 250 is at lane 0 there
    code, part = st.call_cells(lib, tab, case["lnh"], out["ell"], mask, device=device, ens_begin=250, n_ens_out=7)
    assert code == 0 and (part["lnG"][:, :250] == -7.0).all() and (part["cellp"][:, :250] == -7.0).all()
    assert part["lnG"][:, 250:].tobytes() == full["lnG"][:, 250:].tobytes()
    assert part["cellp"][:, 250:].tobytes() == full["cellp"][:, 250:].tobytes()
    # a cell of the grid as the only cell of a call: the first place of the first tile, whatever its place was
    for b in (0, 9, 62, 63):
        one = dict(A=np.ascontiguousarray(tab["A"][b:b + 1]), mx=tab["mx"])
        code, cell = st.call_cells(lib, one, np.ascontiguousarray(case["lnh"][:, b:b + 1]), out["ell"], mask, device=device)
        assert code == 0 and cell["lnG"][0].tobytes() == full["lnG"][b].tobytes(), b
    # and without cellp the same lnG
    code, bare = st.call_cells(lib, tab, case["lnh"], out["ell"], mask, device=device, with_p=False)
    assert code == 0 and bare["lnG"].tobytes() == full["lnG"].tobytes() and (bare["cellp"] == -7.0).all()
