"""iso_binned_compress and iso_binned_lnlike (k_binned_compress, k_binned_rows, k_binned_total) on the device against the
host entries and the twin of tests/_binned_twin.py: M = 35 (fewer samples than lanes), 256 (exactly one tile), 257 (a
one-sample tail) and 800 (a ragged fourth tile); B = 1, 2, 64 and a 3 x 5 grid; H = 1, the row tile, tile + 1 and two tiles
+ 1; both layouts; edge, out, bad and NaN samples in lane 0, lane 255 and the tail; S = 3 with the middle star masked and
S = 257 for the contraction's second block of stars; a second storage with first > 0.  Bit identity: a star alone, in a
batch and in a sub-range, either layout, a repeated call, the rows in one call and in three.  And the identity with
iso_hier_lnlike on FLAT records of the bins."""
import numpy as np
import pytest

from isochrones_amd import _binned_cabi as bc, _hier_cabi as hc, hierarchical as hi, priors as P
from tests import _binned_twin as bt, _hier_twin as tw

pytestmark = pytest.mark.gpu
PM, RM = bt.PM, bt.RM
TILE = bc.ROW_TILE


@pytest.fixture(scope="module")
def lib():
    return bc.lib()


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _special(case):
    """The case with an edge, an out, a bad and a NaN sample in lane 0, lane 255 and the tail of the unmasked stars."""
    x = case["x"].copy()
    M = x.shape[2]
    a0 = case["axes"][0]
    e = case["edges"][0]
    spots = sorted({0, min(255, M - 1), M - 1})
    values = [e[0], e[-1], e[len(e) // 2], np.nextafter(e[-1], 99.0), np.nan]        # first edge, last edge, an edge between, out, NaN
    for i, m in enumerate(spots):
        x[a0, 0, m] = values[i % 5]
        x[a0, -1, m] = values[(i + 3) % 5]
    if M > 4:
        x[a0, 0, 1:4] = e[-1], np.nextafter(e[0], -99.0), np.nan
    return bt.replace_x(case, x)


SHAPES = [(5, 7, (1,), 1, PM), (16, 16, (2,), TILE, RM), (1, 257, (64,), TILE + 1, PM), (32, 25, (3, 5), 2 * TILE + 1, RM),
          (32, 25, (64,), 2 * TILE + 1, PM), (5, 7, (3, 5), TILE + 1, PM), (16, 16, (3, 5), 1, PM), (1, 257, (2,), TILE, RM)]


@pytest.mark.parametrize("W, T, n_bins, H, layout", SHAPES)
def test_device_matches_the_host_entry_and_the_twin(lib, device, W, T, n_bins, H, layout):
    case = _special(bt.make_case(3, W, T, n_bins, H, seed=W + H, layout=layout, n_frozen=1, extra=(W == 16), mask=[1, 0, 1]))
    what = (W, T, n_bins, H, layout)
    htab, hout = bt.run(lib, case)
    dtab, dout = bt.run(lib, case, device=device)
    print(what, "host tables / limit %.3f, device tables / limit %.3f" % (bt.assert_tables_match(htab, case, what),
                                                                         bt.assert_tables_match(dtab, case, what)))
    assert dtab["n_bad"][0] >= 1 and dtab["n_out"][0] >= 1 and np.isnan(dtab["mx"][1]) and not dtab["A"][:, 1].any()
    bt.assert_matches(hout, case, what)
    bt.assert_matches(dout, case, what)
    # and the device against the host entry itself, tables and likelihood
    print(what, "device against host: max |d ell| = %.2e" % bt.assert_device_matches_host(dtab, dout, htab, hout, case, what))
    assert np.isnan(dout["ell"][:, 1]).all() and np.isfinite(dout["L"]).any()
    # L and min_ess are the sums and minima of the device's own star terms
    keep = [0, 2]
    assert np.allclose(dout["L"], dout["ell"][:, keep].sum(axis=1), rtol=1e-14, atol=0)
    assert np.array_equal(dout["min_ess"], dout["ess"][:, keep].min(axis=1))


def test_a_second_block_of_stars_in_the_contraction(lib, device):
    S, H = 257, TILE + 1
    mask = np.ones(S, np.int32)
    mask[[3, 255, 256]] = 0, 1, 1
    case = bt.make_case(S, 5, 7, (4,), H, seed=11, mask=mask)
    dtab, dout = bt.run(lib, case, device=device)
    bt.assert_tables_match(dtab, case)
    bt.assert_matches(dout, case)
    bt.assert_device_matches_host(dtab, dout, *bt.run(lib, case), case, "S = 257")
    assert np.isfinite(dout["ell"][:, 255:]).all() and np.isnan(dout["ell"][:, 3]).all()
    # a star's result does not depend on its block: the last star alone, from a one-star table
    one = {k: np.ascontiguousarray(v[..., 256:]) for k, v in dtab.items()}
    rc, alone = bt.call_lnlike(lib, one, case["lnh"], 35, device=device)
    assert rc == 0 and alone["ell"][:, 0].tobytes() == dout["ell"][:, 256].tobytes()
    assert alone["ess"][:, 0].tobytes() == dout["ess"][:, 256].tobytes()
    # sub-ranges of the stars write their own and leave the rest
    rc, part = bt.call_lnlike(lib, dtab, case["lnh"], 35, mask, device=device, ens_begin=250, n_ens_out=7, total=False)
    assert rc == 0 and (part["ell"][:, :250] == -7.0).all() and part["ell"][:, 250:].tobytes() == dout["ell"][:, 250:].tobytes()


def _same(a, b, keys, stars=slice(None), a_stars=None):
    """The stars ``stars`` of ``b`` are, bit for bit, the stars ``a_stars`` (default: the same) of ``a``."""
    a_stars = stars if a_stars is None else a_stars
    return all(np.ascontiguousarray(a[k][..., a_stars]).tobytes() == np.ascontiguousarray(b[k][..., stars]).tobytes() for k in keys)


TABLES = ("A", "A2", "mx", "n_bad", "n_out")


@pytest.mark.parametrize("W, T, n_bins", [(32, 25, (3, 5)), (1, 257, (64,)), (5, 7, (2,))])
def test_tables_are_bit_identical(lib, device, W, T, n_bins):
    S = 4
    case = _special(bt.make_case(S, W, T, n_bins, 1, seed=5, layout=PM, n_frozen=1))
    rc, full = bt.call_compress(lib, case, device=device)
    assert rc == 0
    assert _same(bt.call_compress(lib, case, device=device)[1], full, TABLES)          # a repeated call
    other = dict(case, layout=RM)
    other["storages"], other["where"] = tw.place(case["x"], W, T, RM, 3)
    assert _same(bt.call_compress(lib, other, device=device)[1], full, TABLES)          # the other layout, other storages
    for s in range(S):                                                                  # a star alone
        alone = bt.replace_x(case, case["x"][:, s:s + 1], S=1)
        assert _same(bt.call_compress(lib, alone, device=device)[1], full, TABLES, slice(s, s + 1), slice(0, 1)), s
    rc, part = bt.call_compress(lib, case, device=device, ens_begin=1, n_ens_out=2)     # a sub-range
    assert rc == 0 and _same(part, full, TABLES, slice(1, 3)) and (part["A"][:, [0, 3]] == -7.0).all()
    assert (part["mx"][[0, 3]] == -7.0).all() and (part["n_bad"][[0, 3]] == -7).all()
    # a derived-style second storage: the stars [1, 3) alone in storages of their own, first = 1
    sub, where = tw.place(case["x"][:, 1:3], W, T, PM, 8)
    n0 = len(case["storages"])
    axis = case["axes"][0]
    cols = [(n0 + k, nc, col, 2, 1) if q == axis else (case["where"][q] + (S, 0)) for q, (k, nc, col) in enumerate(where)]
    rc, moved = bt.call_compress(lib, case, device=device, ens_begin=1, n_ens_out=2, cols=cols, storages=case["storages"] + sub)
    assert rc == 0 and _same(moved, full, TABLES, slice(1, 3))


def test_rows_are_bit_identical_in_any_tiling(lib, device):
    H = 2 * TILE + 1
    case = bt.make_case(5, 5, 7, (3, 5), H, seed=2, mask=[1, 1, 0, 1, 1])
    tab, full = bt.run(lib, case, device=device)
    M = 35
    assert _same(bt.call_lnlike(lib, tab, case["lnh"], M, case["mask"], device=device)[1], full, ("ell", "ess", "L", "min_ess"))
    for lo, hi_ in ((0, TILE), (TILE, TILE + 1), (TILE + 1, H)):
        rc, part = bt.call_lnlike(lib, tab, case["lnh"][lo:hi_], M, case["mask"], device=device)
        assert rc == 0
        for k in ("ell", "ess", "L", "min_ess"):
            assert part[k].tobytes() == full[k][lo:hi_].tobytes(), (k, lo, hi_)


@pytest.mark.parametrize("K", [1, 3])
def test_identity_with_the_hierarchical_library_on_the_device(lib, device, K):
    """test_binned_host_abi_cpu's identity, device against device: ell of a histogram row is logsumexp over the bins of
    lnh_b + ln width_b + ell_b, ell_b from iso_hier_lnlike on the FLAT record of bin b"""
    rng = np.random.default_rng(K)
    S, W, T = 3, 16, 17
    M = W * T
    edges = np.array([0.0, 4.0]) if K == 1 else np.array([0.0, 0.7, 2.5, 4.0])
    x = rng.uniform(-0.5, 4.5, (1, S, M))
    x[0, 0, [0, 255]] = edges[0], edges[-1]
    xs = np.concatenate([x, rng.uniform(0.2, 3.0, (1, S, M))])
    interim = [P.GaussianPrior(2.0, 1.5), P.FlatPrior((0.1, 10.0))]
    pop = P.PowerLawPrior(-2.35, (0.1, 10.0))
    lnh = bt.random_lnh(rng, 4, K)
    case = dict(x=xs, interim=np.concatenate([hi.prior_record(p) for p in interim]),
                frozen=np.concatenate([hi.records(1), hi.prior_record(pop)]), frozen_cols=(1,), axes=(0,), edges=[edges], S=S, W=W,
                T=T, layout=PM, mask=None, extra=None, lnh=lnh)
    case["storages"], case["where"] = tw.place(xs, W, T, PM, 0)
    _, got = bt.run(lib, case, device=device)
    flat = tw.fixed_case(xs, interim, [[P.FlatPrior((edges[b], edges[b + 1])), pop] for b in range(K)], W, T)
    rc, ref = tw.call(hc.lib(), flat, device=device)
    assert rc == 0
    with np.errstate(all="ignore"):
        terms = lnh[:, :, None] + np.log(np.diff(edges))[None, :, None] + ref["ell"][None, :, :]
        want = np.logaddexp.reduce(terms, axis=1)
    fin = np.isfinite(want)
    assert fin.any() and np.array_equal(np.isfinite(got["ell"]), fin)
    d = np.abs(got["ell"] - want)[fin]
    print("K = %d: max |d ell| = %.2e" % (K, d.max()))
    assert np.all(d <= 1e-11)
