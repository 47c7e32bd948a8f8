"""The DFInterpolator kernels (k_interp<2|3|4>, k_interp3_wide<8|4>, the one-point paths) on the edge tables of
tests/_interp_twin.py, against the long-double twin of the reference's rule: uniform axes whose step is no power of two (the
O(1) index and its ++k / --k fix-up, with NaN nodes placed so that a wrong cell shows), axes that do not fit the LDS budget
(bisected in global memory) or fill it exactly, two nodes on every axis, every mapping of columns to lanes, and the second
and third trip of the capped grid; then the fused kernels' EEP bracket (fast/brackets.h) on an exactly uniform, non-integer EEP
axis and a model whose mass axis is beyond the LDS budget, against the CPU oracle.  For the DFInterpolator kernels the NaN pattern must be exact and every value within

    2 * (5*ND + 2**ND + 1) * 2**-53 * sum_j |v_j|

(derived in the twin's docstring).  Every test prints the worst error / limit it saw."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _cabi, device as dev
from isochrones_amd.interp import DFInterpolator
from tests import _interp_twin as tw

pytestmark = pytest.mark.gpu

_TABLES = {}


def table(t):
    if t.name not in _TABLES:
        _TABLES[t.name] = DFInterpolator.from_arrays(t.grid, t.axes, t.columns)
    return _TABLES[t.name]


def on_device(dfi, xs, icols):
    import torch
    xt = [torch.as_tensor(np.ascontiguousarray(x), device="cuda") for x in xs]
    _cabi.trace_kernels(True)
    try:
        out = dfi.interp_device(xt, np.asarray(icols, dtype=np.int32)).cpu().numpy()
        names = _cabi.traced_kernels()
    finally:
        _cabi.trace_kernels(False)
    return out, names


def tiled(t, n):
    """n probes: the table's, repeated."""
    rows = np.arange(n) % t.probes.shape[0]
    return t.xs(rows)


def bits(a):
    return np.ascontiguousarray(np.nan_to_num(np.asarray(a, dtype=np.float64), nan=7.25))


ALL = list(tw.UNIFORM) + list(tw.UNSTAGED) + list(tw.MINIMUM)


@pytest.mark.parametrize("name", ALL)
def test_column_parallel_kernel_on_every_edge_table(name, monkeypatch):
    monkeypatch.setenv("ISOCHRONES_AMD_PATH", "generic")           # (a 3-D table: no wide pack)
    t = tw.edge_table(name)
    dfi = table(t)
    icols = np.arange(t.ncol)
    got, names = on_device(dfi, t.xs(), icols)
    assert "k_interp<%d>" % t.nd in names, names
    worst = tw.check(got, t.grid, t.axes, t.xs(), icols, name)
    for n in (1, 63, 64, 65, 257):
        part, _ = on_device(dfi, t.xs(np.arange(n)), icols)
        assert np.array_equal(bits(part), bits(got[:n])), (name, n)
    print("%s: k_interp<%d> worst error / limit %.3g over %d probes" % (name, t.nd, worst, got.shape[0]))


@pytest.mark.parametrize("name", ["U3", "G3_global", "G3_exact"])
def test_wide_pack_kernels_on_the_3d_edge_tables(name, monkeypatch):
    monkeypatch.setenv("ISOCHRONES_AMD_PATH", "auto")
    t = tw.edge_table(name)
    dfi = DFInterpolator.from_arrays(t.grid, t.axes, t.columns)    # a table of its own: the pack is built by this batch
    n = 32768 + 77
    xs = tiled(t, n)
    for icols in ([np.arange(t.ncol)] if t.ncol > 1 else []) + [np.array([t.ncol - 1])]:
        got, names = on_device(dfi, xs, icols)
        kernel = "k_interp3_wide<%d>" % (4 if icols.size == 1 else 8)
        assert kernel in names, names
        worst = tw.check(got, t.grid, t.axes, xs, icols, name + " " + kernel)
        print("%s: %s worst error / limit %.3g over %d rows" % (name, kernel, worst, n))
    dfi.release()


@pytest.mark.parametrize("name", ALL)
def test_one_point_calls_are_the_launch_path_bit_for_bit(name, monkeypatch):
    t = tw.edge_table(name)
    dfi = table(t)
    cols = t.columns
    rows = np.arange(48)
    pts = [[float(v) for v in t.probes[r]] for r in rows]
    monkeypatch.delenv("ISOCHRONES_AMD_MAILBOX", raising=False)    # the context's resident service wave
    one = np.array([dfi(p, cols) for p in pts])
    monkeypatch.setenv("ISOCHRONES_AMD_MAILBOX", "0")              # a launch per point
    launched = np.array([dfi(p, cols) for p in pts])
    assert np.array_equal(bits(one), bits(launched)), name
    batch = dfi([t.probes[rows, d] for d in range(t.nd)], cols)    # one small host batch
    assert np.array_equal(bits(one), bits(batch)), name
    worst = tw.check(one, t.grid, t.axes, t.xs(rows), np.arange(t.ncol), name + " one point at a time")
    assert np.isnan(one).any() and np.isfinite(one).any()
    print("%s: one-point calls worst error / limit %.3g" % (name, worst))


def test_a_table_of_257_columns_takes_the_launch_path():
    t = tw.widen(tw.edge_table("U2"), 257)
    dfi = DFInterpolator.from_arrays(t.grid, t.axes, t.columns)
    icols = np.array([0, 128, 256, 5])
    cols = ["c%d" % j for j in icols]
    rows = np.arange(40)
    _cabi.trace_kernels(True)
    try:
        one = np.array([dfi([float(v) for v in t.probes[r]], cols) for r in rows])
        names = _cabi.traced_kernels()
    finally:
        _cabi.trace_kernels(False)
    assert "k_interp<2>" in names and "k_service" not in names, names
    batch, _ = on_device(dfi, t.xs(rows), icols)
    assert np.array_equal(bits(one), bits(batch))
    worst = tw.check(one, t.grid, t.axes, t.xs(rows), icols, "257 columns")
    print("257 columns: worst error / limit %.3g" % worst)
    dfi.release()


@pytest.fixture(scope="module")
def wide_tables():
    out = {}
    for name in ("U2", "U4"):
        t = tw.widen(tw.edge_table(name), 70)
        out[name] = (t, DFInterpolator.from_arrays(t.grid, t.axes, t.columns))
    yield out
    for _, dfi in out.values():
        dfi.release()


def samples_per_wave(k):
    return 64 // ((k + 1) // 2)


@pytest.mark.parametrize("k", [1, 2, 3, 9, 43, 63, 64])
@pytest.mark.parametrize("name", ["U2", "U4"])
def test_every_mapping_of_columns_to_lanes(name, k, wide_tables):
    t, dfi = wide_tables[name]
    rng = np.random.default_rng(100 * k + t.nd)
    S = samples_per_wave(k)
    worst = 0.0
    for n in (S - 1, S, S + 1, t.probes.shape[0]):
        if n == 0:
            continue
        icols = rng.choice(t.ncol, size=k, replace=False)
        xs = t.xs(np.arange(n))
        got, names = on_device(dfi, xs, icols)
        assert "k_interp<%d>" % t.nd in names
        worst = max(worst, tw.check(got, t.grid, t.axes, xs, icols, "%s k=%d n=%d" % (name, k, n)))
    print("%s: k = %d (S = %d) worst error / limit %.3g" % (name, k, S, worst))


@pytest.mark.parametrize("name", ["U2", "U4"])
def test_repeated_and_descending_column_indices_and_k_65(name, wide_tables):
    t, dfi = wide_tables[name]
    xs = t.xs()
    worst = 0.0
    for icols in ([5, 5, 69, 3, 3, 2, 1, 0, 0], list(range(69, 26, -1)), [7, 7]):
        got, _ = on_device(dfi, xs, np.array(icols))
        worst = max(worst, tw.check(got, t.grid, t.axes, xs, np.array(icols), "%s icols=%s" % (name, icols[:4])))
    print("%s: repeated / descending columns worst error / limit %.3g" % (name, worst))
    # 65 columns in one call: refused by the library (the Python layer splits such a call before it gets there)
    import torch
    xt = [torch.as_tensor(x[:4].copy(), device="cuda") for x in xs]
    out = torch.full((4, 65), 3.0, dtype=torch.float64, device="cuda")
    ic = np.arange(65, dtype=np.int32)
    xp = (C.c_void_p * t.nd)(*[x.data_ptr() for x in xt])
    device = xt[0].device.index
    rc = _cabi.lib().iso_interp(dfi.handle(device), xp, 4, ic.ctypes.data_as(C.POINTER(C.c_int32)), 65, dev.ptr(out),
                                dev.stream_ptr(device))
    assert rc == _cabi.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


@pytest.mark.parametrize("k", [64, 1])
def test_second_and_third_trip_of_the_wave_stride_loop(k, wide_tables):
    t, dfi = wide_tables["U2"]
    T = _cabi.ISO_MAX_GRID_BLOCKS * 4 * samples_per_wave(k)        # samples of one trip: 2048 workgroups of four waves
    assert T == {64: 16384, 1: 524288}[k]
    icols = np.arange(3, 3 + k)
    for n in (T + 1, 2 * T + 3):
        xs = tiled(t, n)
        got, names = on_device(dfi, xs, icols)
        assert "k_interp<2>" in names
        worst = tw.check(got, t.grid, t.axes, xs, icols, "k=%d n=%d" % (k, n))
        print("U2: k = %d, n = %d (T = %d) worst error / limit %.3g" % (k, n, T, worst))


# ---- the fused bracket (fast/brackets.h: eep_bracket) and a model beyond the LDS budget --------------------------------------
RTOL, ATOL = 1e-9, 1e-10            # tests/test_gpu_odd_shapes.py
FEHS = np.array([-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5])
N_ROWS = 20_000


def _off_nodes(eeps, lo, hi):
    """Nodes in [lo, hi] where a first guess is off: {(guess name, direction): nodes}.  ++k shows at x = a_j, --k at the
    double below a_j."""
    out = {}
    for guess in (tw.first_guess_generic, tw.first_guess_fused):
        up = tw.fixup_needed(eeps, eeps, guess)
        down = tw.fixup_needed(eeps, np.clip(np.nextafter(eeps, -np.inf), eeps[0], None), guess)
        j = np.arange(eeps.size)
        out[(guess.__name__, 1)] = j[(up == 1) & (j >= lo) & (j <= hi)]
        out[(guess.__name__, -1)] = j[(down == -1) & (j >= lo) & (j <= hi)]
    return out


def _fused_case(kind, n_stars, nb, step):
    """(interpolator, model, rows, model-table coordinates of the rows).  The EEP axis is step * i, i = 0 .. 999: exactly
    uniform and not integer.  Pairs of neighbouring tracks (isochrones) end at a node right above one where a first guess of
    the bracket is off, so that the probes there are decisive; the rows are the EEP at every node and at both its neighbours,
    and the rest around those ragged ends."""
    import isochrones_amd as ia
    from isochrones_amd import grids
    from isochrones_amd.models import (BolometricCorrectionGrid, EvolutionTrackGrid, EvolutionTrackInterpolator, IsochroneGrid,
                                       IsochroneInterpolator)
    rng = np.random.default_rng([20261023, n_stars, nb, int(step * 10)])
    eeps = np.arange(1000, dtype=np.float64) * step
    assert tw.is_uniform(eeps) and eeps[1] != round(eeps[1])
    obs_bands = tuple(ia.grids.DEFAULT_BANDS[:nb])
    with np.errstate(invalid="ignore"):                    # (the toy physics is undefined below EEP 1: NaN nodes, as it happens)
        if kind == "track":
            first = ia.grids.mist_masses()[20:150:3]
            g, ax, cols = grids.synthetic_track_grid(FEHS, first, eeps)
            pair_axis, lo_node, hi_node = 1, (150 if step > 0.5 else 20), (640 if step > 0.5 else 990)
        else:
            first = ia.grids.mist_log_ages()[40::3]
            g, ax, cols = grids.synthetic_iso_grid(first, FEHS, eeps)
            pair_axis, lo_node, hi_node = 0, 300, 990
    off = _off_nodes(eeps, lo_node, hi_node)
    picks = []
    for key in sorted(off):                                # four ragged ends per (guess, direction) that occurs on this axis
        nodes = off[key]
        if nodes.size:
            picks += [int(v) for v in nodes[np.linspace(0, nodes.size - 1, 4).astype(int)]]
    picks = picks[: first.size // 2]
    for p, j in enumerate(picks):                          # tracks 2p and 2p + 1 end at node j: node j + 1 onwards is missing
        sl = [slice(None)] * 3
        sl[pair_axis] = slice(2 * p, 2 * p + 2)
        sl[2] = slice(j + 1, None)
        g[tuple(sl)] = np.nan
    bg, bax, bbands = grids.synthetic_bc_grid(obs_bands)
    bcg = BolometricCorrectionGrid(DFInterpolator.from_arrays(bg, bax, list(bbands)), bands=obs_bands)
    if kind == "track":
        mg = EvolutionTrackGrid(DFInterpolator.from_arrays(g, ax, list(cols), ["initial_feh", "initial_mass", "EEP"]),
                                limits=dict(mass=(first[0], first[-1]), feh=(-2.0, 0.5), age=(5, 10.13)))
        ic = EvolutionTrackInterpolator(mg, bcg, bands=obs_bands, eep_bounds=(eeps[0], eeps[-1]))
        lo = np.array([first[0], eeps[0], -2.0, 5.0, 0.0])
        hi = np.array([first[-1], eeps[-1], 0.5, 2000.0, 1.0])
        c_first, c_feh, c_eep = 0, 2, 1
    else:
        mg = IsochroneGrid(DFInterpolator.from_arrays(g, ax, list(cols), ["log10_isochrone_age_yr", "feh", "EEP"]),
                           limits=dict(age=(first[0], first[-1]), feh=(-2.0, 0.5)))
        ic = IsochroneInterpolator(mg, bcg, bands=obs_bands, eep_bounds=(eeps[0], eeps[-1]))
        lo = np.array([eeps[0]] * n_stars + [first[0], -2.0, 5.0, 0.0])
        hi = np.array([eeps[-1]] * n_stars + [first[-1], 0.5, 2000.0, 1.0])
        c_first, c_feh, c_eep = n_stars, n_stars + 1, 0
    obs = dict(Teff=(5770, 100), logg=(4.4, 0.1), feh=(0.0, 0.15), parallax=(2.0, 0.05))
    for j, b in enumerate(obs_bands):
        obs[b] = (10.0 + 0.1 * j, 0.02)
    mod = ia.BasicStarModel(ic, N=n_stars, **obs)
    # rows
    pars = rng.uniform(lo, hi, size=(N_ROWS, lo.size))
    nodes = np.concatenate([eeps, np.nextafter(eeps, -np.inf), np.nextafter(eeps, np.inf)])
    pars[:nodes.size, c_eep] = nodes                       # every node and both neighbours (so: one ulp outside either end)
    pars[nodes.size:nodes.size + 4, c_eep] = [np.nan, 0.0, -0.0, eeps[-1]]
    at = nodes.size + 4
    per = (N_ROWS - at) // max(1, len(picks))
    for p, j in enumerate(picks):                          # between the two tracks that end at node j, around that node
        rows = slice(at + p * per, at + (p + 1) * per)
        pars[rows, c_first] = rng.uniform(first[2 * p], first[2 * p + 1], per)
        e = rng.uniform(eeps[j - 2], eeps[j + 2], per)
        e[0::4] = eeps[j]
        e[1::4] = np.nextafter(eeps[j], -np.inf)
        e[2::8] = np.nextafter(eeps[j], np.inf)
        pars[rows, c_eep] = e
    if n_stars > 1:                                        # the secondary below the primary, on populated nodes
        pars[:, 1] = np.minimum(pars[:, 1], pars[:, 0])
    coords = [pars[:, c_first], pars[:, c_feh], pars[:, c_eep]]
    if kind == "track":
        coords = [pars[:, c_feh], pars[:, c_first], pars[:, c_eep]]
    return ic, mod, pars, (g, ax, coords), obs_bands


@pytest.fixture(params=["auto", "compact", "generic"])
def kernel_path(request, monkeypatch):
    monkeypatch.setenv("ISOCHRONES_AMD_PATH", request.param)
    return request.param


@pytest.mark.parametrize("kind,n_stars,nb,step", [("track", 1, 1, 0.7), ("track", 1, 3, 0.7), ("iso", 1, 1, 0.7), ("iso", 1, 3, 0.7),
                                                  ("iso", 2, 1, 0.7), ("iso", 2, 3, 0.7), ("track", 1, 1, 0.1), ("track", 1, 3, 0.1)])
def test_fused_bracket_on_a_uniform_non_integer_eep_axis(kind, n_stars, nb, step, kernel_path):
    """eep_bracket()'s O(1) index and its fix-up (auto, compact) and bracket()'s in the generic lnpost kernel, against the CPU
    oracle.  The decisive probes are counted by the twin under the guess of the kernel that runs.  On a_i = 0.7 i the fused
    guess is never too high (tests/test_interp_twin_cpu.py), so its --k is reached by the a_i = 0.1 i cases, where it is
    never too low; the generic guess errs both ways on either axis."""
    from tests import _fixtures as fx
    ic, mod, pars, (g, ax, coords), bands = _fused_case(kind, n_stars, nb, step)
    if kernel_path == "auto":
        assert mod.kernel_path() == "fused-packed"
    gen = tw.fixup_counts_on(g, ax, coords, 2, tw.first_guess_generic)
    fus = tw.fixup_counts_on(g, ax, coords, 2, tw.first_guess_fused)
    print("%s N=%d %d bands step %.1f %s (%s): decisive ++ / -- generic guess %d / %d, fused guess %d / %d" % (
        kind, n_stars, nb, step, kernel_path, mod.kernel_path(), gen[0], gen[1], fus[0], fus[1]))
    assert gen[0] >= 3 and gen[1] >= 3, gen
    assert (fus[0] >= 3 and fus[1] == 0) if step > 0.5 else (fus[1] >= 3 and fus[0] == 0), fus
    oic = fx.make_oracle_ic(ic)
    w_post, w_prior, w_like = oic.lnpost(mod.model_desc(), pars.T.copy(), nthreads=8)
    assert np.isfinite(w_post).sum() > N_ROWS // 100
    fx.assert_close(mod.lnpost(pars), w_post, RTOL, atol=ATOL, what="lnpost")
    fx.assert_close(mod.lnprior(pars), w_prior, RTOL, atol=ATOL, what="lnprior")
    fx.assert_close(mod.lnlike(pars), w_like, RTOL, atol=ATOL, what="lnlike")
    prim = np.column_stack([pars[:, 0]] + [pars[:, n_stars + j] for j in range(4)]).T.copy()
    wT, wg, wf, wm = oic.interp_mag(prim, [ic.bc_grid.interp.column_index[b] for b in bands], nthreads=8)
    T, g_, f, m = ic.interp_mag(list(prim), list(bands))
    fx.assert_close(T, wT, RTOL, what="Teff")
    fx.assert_close(m, wm, RTOL, atol=ATOL, what="mags")


def test_fused_sampler_on_a_uniform_non_integer_eep_axis():
    """The sampler kernels share eep_bracket(): the stored lnprob of a 60-step run equals the oracle's lnpost of the stored
    positions."""
    from isochrones_amd.sampler import FusedEnsembleSampler
    from tests import _fixtures as fx
    ic, mod, _, _, _ = _fused_case("track", 1, 3, 0.7)
    assert mod.kernel_path() == "fused-packed"
    rng = np.random.default_rng(11)
    masses = ic.model_grid.interp.index_columns[1]
    truth = np.array([0.5 * (masses[-5] + masses[-4]), 355.0, 0.0, 480.0, 0.1])      # between two tracks that were not cut short
    x = truth + np.array([0.01, 2.0, 0.02, 4.0, 0.02]) * rng.standard_normal((512, 5))
    x[:, 4] = np.abs(x[:, 4])
    good = np.flatnonzero(np.isfinite(mod.lnpost(x)))
    assert good.size >= 64, good.size
    p0 = x[good[:64]]
    fs = FusedEnsembleSampler(mod, 64, seed=3)
    fs.run_mcmc(p0, 60, store=True)
    chain = fs.chain_steps.cpu().numpy().reshape(-1, 5)
    want = fx.make_oracle_ic(ic).lnpost(mod.model_desc(), chain.T.copy(), parts=False)
    fx.assert_close(fs._lnprob.cpu().numpy().reshape(-1), want, RTOL, atol=ATOL, what="sampler lnprob on the 0.7 i axis")


def test_a_model_whose_mass_axis_is_beyond_the_lds_budget():
    """A track table with 6200 non-uniform masses (3 fehs, 20 EEPs): its axes do not fit the fused kernels' LDS blob, so the
    library must pick another path, and that path must be right."""
    import isochrones_amd as ia
    from tests import _fixtures as fx
    rng = np.random.default_rng(6200)
    masses = np.unique(np.sort(rng.uniform(0.7, 3.0, 6200)))
    assert masses.size == 6200 and not tw.is_uniform(masses)
    fehs, eeps = np.array([-0.5, 0.0, 0.4]), np.arange(300.0, 320.0)
    bands = tuple(ia.grids.DEFAULT_BANDS[:3])
    ic = ia.synthetic_track(bands=bands, fehs=fehs, masses=masses, eeps=eeps, eep_bounds=(eeps[0], eeps[-1]),
                            limits=dict(mass=(masses[0], masses[-1]), feh=(-0.5, 0.4), age=(5, 10.13)))
    obs = dict(Teff=(5770, 100), logg=(4.4, 0.1), feh=(0.0, 0.15), parallax=(2.0, 0.05), G=(10.0, 0.02), BP=(10.1, 0.02),
               RP=(10.2, 0.02))
    obs = {k: v for k, v in obs.items() if k in bands or k in ("Teff", "logg", "feh", "parallax")}
    mod = ia.BasicStarModel(ic, N=1, **obs)
    path = mod.kernel_path()
    print("6200 masses: kernel path %s" % path)
    assert path != "fused-packed"
    lo = np.array([masses[0], eeps[0], -0.5, 5.0, 0.0])
    hi = np.array([masses[-1], eeps[-1], 0.4, 2000.0, 1.0])
    pars = rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo), size=(N_ROWS, 5))
    pars[:6200, 0] = masses                                # every node of the long axis, and neighbours of some
    pars[6200:9200, 0] = np.nextafter(masses[:3000], -np.inf)
    pars[9200:12200, 0] = np.nextafter(masses[3200:], np.inf)
    pars[12200:12210, 0] = np.nan
    oic = fx.make_oracle_ic(ic)
    w_post, w_prior, w_like = oic.lnpost(mod.model_desc(), pars.T.copy(), nthreads=8)
    assert np.isfinite(w_post).sum() > N_ROWS // 10
    fx.assert_close(mod.lnpost(pars), w_post, RTOL, atol=ATOL, what="lnpost, 6200 masses")
    prim = pars.T.copy()
    prim[3] = np.abs(prim[3]) + 1.0
    wT, wg, wf, wm = oic.interp_mag(prim, [ic.bc_grid.interp.column_index[b] for b in bands], nthreads=8)
    T, g_, f, m = ic.interp_mag(list(prim), list(bands))
    fx.assert_close(T, wT, RTOL, what="Teff")
    fx.assert_close(m, wm, RTOL, atol=ATOL, what="mags")
