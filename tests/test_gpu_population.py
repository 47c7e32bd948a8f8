"""libiso_population.so on the device: the kernel against the host entry of the same library (model columns bit for bit,
magnitudes and extinctions within 1e-9, identical NaN patterns) over the shapes at which the kernel takes another path,
batch independence, no stray writes, a non-default stream, batches at and beyond the grid's cap; then the Python layer end to end against the independent path
through ``interp_value`` / ``interp_mag`` (``ic.generate_binary``), the twin and the golden from the reference."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _population_twin as tw

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dt(Q, B):
    return tw.DeviceTables(tw.tables(Q, B))


@functools.lru_cache(maxsize=None)
def _host(Q, B, N, Cn):
    """The reference of the device tests, computed once per shape."""
    x, d, a = tw.inputs(N, Cn)
    return tw.host(tw.tables(Q, B), x, d, a)


@pytest.mark.parametrize("N", tw.NS)
@pytest.mark.parametrize("Cn", (1, 2))
def test_device_equals_host_over_batch_sizes(N, Cn):
    x, d, a = tw.inputs(N, Cn)
    tw.assert_same(tw.device(_dt(18, 7), x, d, a), _host(18, 7, N, Cn), "N=%d C=%d" % (N, Cn))


@pytest.mark.parametrize("Q", tw.QS)
@pytest.mark.parametrize("B", tw.BS)
@pytest.mark.parametrize("Cn", (1, 2))
def test_device_equals_host_over_columns_and_bands(Q, B, Cn):
    x, d, a = tw.inputs(257, Cn)
    want = _host(Q, B, 257, Cn)
    tw.assert_same(tw.device(_dt(Q, B), x, d, a), want, "Q=%d B=%d C=%d" % (Q, B, Cn))
    assert np.isnan(want["sys_mag"]).any() and np.isfinite(want["sys_mag"]).any()


@pytest.mark.parametrize("Q,B", tw.WIDE)
def test_device_equals_host_beyond_one_pass_of_bands(Q, B):
    x, d, a = tw.inputs(257, 2)
    tw.assert_same(tw.device(_dt(Q, B), x, d, a), _host(Q, B, 257, 2), "Q=%d B=%d" % (Q, B))
    x, d, a = tw.inputs(65, 1)
    tw.assert_same(tw.device(_dt(Q, B), x, d, a), _host(Q, B, 65, 1), "Q=%d B=%d C=1" % (Q, B))


def test_device_equals_twin():
    x, d, a = tw.inputs(1000, 2)
    tw.assert_same(tw.device(_dt(18, 7), x, d, a), tw.evaluate(tw.tables(18, 7), x, d, a), "twin")


def test_a_system_does_not_depend_on_its_batch():
    """Alone, first, last and in the middle of a batch; and from a call on a sub-range: distance and AV are pointers into the
    larger arrays (an odd offset), the coordinates - whose stride is the batch size - the packed rows of the range."""
    import torch
    from isochrones_amd import _population_cabi as pc, device as dev
    dt = _dt(18, 7)
    x, d, a = tw.inputs(257, 2)
    full = tw.device(dt, x, d, a)
    for i in (0, 1, 70, 128, 256):
        one = tw.device(dt, np.ascontiguousarray(x[:, :, i:i + 1]), d[i:i + 1].copy(), a[i:i + 1].copy())
        for k in tw.OUTPUTS:
            assert tw.same_bits(one[k][..., 0], full[k][..., i]), (i, k)
    lo, n = 37, 131
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")      # noqa: E731
    d_x, d_d, d_a = up(x[:, :, lo:lo + n]), up(d), up(a)
    bufs = {k: tw.guarded(s) for k, s in tw.shapes(2, 18, 7, n).items()}
    out = pc.IsoPopulationOut(*[dev.ptr(bufs[k][1]) for k in tw.OUTPUTS])
    pc.check(pc.lib().iso_population_eval(C.byref(dt.model), C.byref(dt.bct), dev.ptr(d_x), d_d.data_ptr() + 8 * lo,
                                          d_a.data_ptr() + 8 * lo, n, 2, C.byref(out), dev.stream_ptr(0)))
    torch.cuda.synchronize()
    for k in tw.OUTPUTS:
        assert tw.margins_untouched(bufs[k][0]), k
        assert tw.same_bits(bufs[k][1].cpu().numpy(), full[k][..., lo:lo + n]), k


BLOCK = 256                                                      # lanes of a workgroup


def _cap():
    from isochrones_amd import _population_cabi as pc
    return pc.MAX_BLOCKS * BLOCK                                 # systems of one trip of the capped grid


@pytest.mark.parametrize("trips", ("cap", "cap_plus_1", "two_caps_plus_65"))
@pytest.mark.parametrize("Cn", (1, 2))
@pytest.mark.parametrize("Q, B", ((4, 1), (18, 7)))
def test_the_second_and_third_trip_of_the_stride_loop(Q, B, Cn, trips):
    """N = CAP (every lane one system, the loop's exit test alone), CAP + 1 (lane 0 of workgroup 0 a second one) and
    2 * CAP + 65 (a third trip of 65 lanes), CAP = ISO_POPULATION_MAX_BLOCKS * 256.

    Compared with the host entry in full where that takes under a second for the 1.05e6 systems of 2 * CAP + 65 (measured
    on one CPU core: Q = 4, B = 1 0.6 s single or binary, Q = 18, B = 7 single 0.9 s).  Q = 18, B = 7 binaries take it 2.6 s
    and give 0.65 GB of outputs, so they are compared on three windows that contain every boundary between two trips:
    [0, 513), [CAP - 256, CAP + 257) and the last 513 systems (clipped to the batch).  Everywhere: no sentinel is left in
    an output (a system skipped), the margins are untouched (``device_tensors``), and the systems either side of the
    first trip's end have the bits of a call on them alone."""
    import torch
    from isochrones_amd import _population_cabi as pc, device as dev
    CAP = _cap()
    assert pc.MAX_BLOCKS == 2048
    N = {"cap": CAP, "cap_plus_1": CAP + 1, "two_caps_plus_65": 2 * CAP + 65}[trips]
    dt, tab = _dt(Q, B), tw.tables(Q, B)
    x, d, a = tw.inputs(N, Cn)
    got = tw.device_tensors(dt, x, d, a)
    for k in tw.OUTPUTS:
        assert got[k].shape == tw.shapes(Cn, Q, B, N)[k] and not bool((got[k] == tw.SENTINEL).any()), k
    if (Q, B, Cn) != (18, 7, 2):
        windows = [(0, N)]
    else:
        windows = sorted({(0, 513), (CAP - 256, min(N, CAP + 257)), (N - 513, N)})
    for lo, hi in windows:
        want = tw.host(tab, np.ascontiguousarray(x[:, :, lo:hi]), d[lo:hi], a[lo:hi])
        tw.assert_same({k: got[k][..., lo:hi].cpu().numpy() for k in tw.OUTPUTS}, want,
                       "Q=%d B=%d C=%d N=%d [%d, %d)" % (Q, B, Cn, N, lo, hi))
    # a call on the sub-range alone: distance and AV are pointers into the larger arrays, the coordinates its packed rows
    lo, hi = CAP - 64, min(N, CAP + 65)
    n = hi - lo
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")      # noqa: E731
    d_x, d_d, d_a = up(x[:, :, lo:hi]), up(d), up(a)
    bufs = {k: tw.guarded(s) for k, s in tw.shapes(Cn, Q, B, n).items()}
    out = pc.IsoPopulationOut(*[dev.ptr(bufs[k][1]) for k in tw.OUTPUTS])
    pc.check(pc.lib().iso_population_eval(C.byref(dt.model), C.byref(dt.bct), dev.ptr(d_x), d_d.data_ptr() + 8 * lo,
                                          d_a.data_ptr() + 8 * lo, n, Cn, C.byref(out), dev.stream_ptr(0)))
    torch.cuda.synchronize()
    for k in tw.OUTPUTS:
        assert tw.margins_untouched(bufs[k][0]), k
        # (as 64-bit patterns: the NaNs of an off-grid system are the same bits too)
        assert torch.equal(bufs[k][1].view(torch.int64), got[k][..., lo:hi].contiguous().view(torch.int64)), k


def test_null_outputs_stay_unwritten_and_margins_untouched():
    dt = _dt(9, 3)
    x, d, a = tw.inputs(65, 2)
    full = tw.device(dt, x, d, a)                               # (device() itself checks the margins of every output)
    for want in (("sys_mag",), ("cols_out",), ("A_out", "sys_A"), ("mag_out",), ()):
        got = tw.device(dt, x, d, a, want=want)
        for k in tw.OUTPUTS:
            if k in want:
                assert tw.same_bits(got[k], full[k]), (want, k)
            else:
                assert (got[k] == tw.SENTINEL).all(), (want, k)


def test_n_zero_and_argument_errors_launch_nothing():
    import torch
    from isochrones_amd import _population_cabi as pc, device as dev
    dt = _dt(8, 3)
    flat, view = tw.guarded((2, 8, 4))
    out = pc.IsoPopulationOut(dev.ptr(view), None, None, None, None)
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    L = pc.lib()
    assert L.iso_population_eval(C.byref(dt.model), C.byref(dt.bct), dev.ptr(z), dev.ptr(z), dev.ptr(z), 0, 2, C.byref(out),
                                 dev.stream_ptr(0)) == 0
    assert L.iso_population_eval(C.byref(dt.model), C.byref(dt.bct), dev.ptr(z), dev.ptr(z), dev.ptr(z), 4, 3, C.byref(out),
                                 dev.stream_ptr(0)) == pc.ERR_INVALID
    assert L.iso_population_last_error().decode() == "iso_population_eval: C must be 1 or 2 components"
    odd = pc.IsoPopulationModelTable.from_buffer_copy(dt.model)
    odd.cols = dt.model.cols + 8
    assert L.iso_population_eval(C.byref(odd), C.byref(dt.bct), dev.ptr(z), dev.ptr(z), dev.ptr(z), 4, 2, C.byref(out),
                                 dev.stream_ptr(0)) == pc.ERR_INVALID
    assert "16-byte aligned" in L.iso_population_last_error().decode()
    torch.cuda.synchronize()
    assert bool((flat == tw.SENTINEL).all())


def test_runs_on_the_given_stream():
    """On a non-default stream, followed by a dependent torch op on that stream without a synchronise in between."""
    import torch
    from isochrones_amd import _population_cabi as pc, device as dev
    dt = _dt(18, 7)
    x, d, a = tw.inputs(1000, 2)
    want = _host(18, 7, 1000, 2)
    d_x, d_d, d_a = (torch.as_tensor(np.ascontiguousarray(v), device="cuda") for v in (x, d, a))
    sm = torch.full((7, 1000), tw.SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = pc.IsoPopulationOut(None, None, None, dev.ptr(sm), None)
        pc.check(pc.lib().iso_population_eval(C.byref(dt.model), C.byref(dt.bct), dev.ptr(d_x), dev.ptr(d_d), dev.ptr(d_a),
                                              1000, 2, C.byref(out), s.cuda_stream))
        twice = sm * 2.0
    s.synchronize()
    ok, dev_ = tw.close(twice.cpu().numpy(), 2.0 * want["sys_mag"])
    assert ok, dev_


# ---- the Python layer end to end ----------------------------------------------------------------------------------------------

def _pairs(n, seed=7):
    rng = np.random.default_rng(seed)
    mass_A = rng.uniform(0.4, 1.3, n)
    mass_B = np.where(rng.integers(0, 4, n) == 0, 0.0, mass_A * rng.uniform(0.3, 1.0, n))
    return (mass_A, mass_B, rng.uniform(8.0, 8.6, n), rng.uniform(-1.0, 0.5, n), rng.uniform(20.0, 900.0, n),
            rng.uniform(0.0, 1.0, n))


@pytest.mark.parametrize("shared_eeps", (False, True))
def test_evaluate_binaries_equals_generate_binary(shared_eeps):
    """Against the independent path through interp_value and interp_mag (``ic.generate_binary``), on the same inputs; with
    ``shared_eeps`` on the same given EEPs too (``generate_binary`` hands one ``eeps`` to both components)."""
    import torch
    import isochrones_amd as ia
    ic = tw.small_ic()
    n = 257
    mA, mB, age, feh, dist, av = _pairs(n)
    kw = {}
    eeps = None
    if shared_eeps:
        e = np.random.default_rng(8).uniform(421.0, 466.0, n)
        kw, eeps = dict(eeps=e), (torch.as_tensor(e, device="cuda"), torch.as_tensor(e, device="cuda"))
    want = ic.generate_binary(mA, mB, age, feh, distance=dist, AV=av, all_As=True, **kw)
    up = lambda v: torch.as_tensor(v, device="cuda")                            # noqa: E731
    got = ia.evaluate_binaries(ic, up(mA), up(mB), up(age), up(feh), up(dist), up(av), eeps=eeps)
    assert all(t.is_cuda and t.dtype == torch.float64 and t.shape == (n,) for t in got.values())
    shared = [c for c in want.columns if c in got]
    assert len(shared) == len(want.columns) == len(got) - 7      # all but the system's A_<band>
    assert np.isfinite(want["V_mag"].values).sum() > 100 and np.isnan(want["V_mag_1"].values).sum() > 30
    for c in shared:
        ok, dev_ = tw.close(got[c].cpu().numpy(), want[c].values)
        assert ok, (c, dev_)
    # the system's extinctions: the twin, on the EEPs the device path used
    m, names = ic.model_grid.interp, list(ic.model_grid.interp.columns)
    tab = (np.ascontiguousarray(m.grid, dtype=np.float64), tuple(m.index_columns), tuple(int(i) for i in ic._cols),
           np.ascontiguousarray(ic.bc_grid.interp.grid[..., [int(i) for i in ic._band_cols(list(ic.bands))]]),
           tuple(ic.bc_grid.interp.index_columns))
    assert names[tab[2][0]] == "Teff"
    coords = np.array([[feh, mA, got["eep_0"].cpu().numpy()], [feh, mB, got["eep_1"].cpu().numpy()]])
    if not shared_eeps:                                          # (an off-grid star's eep column is NaN whatever its EEP was)
        coords[0, 2] = ic.get_eep(mA, age, feh)
        coords[1, 2] = ic.get_eep(mB, age, feh)
    else:
        coords[0, 2] = coords[1, 2] = kw["eeps"]
    w = tw.evaluate(tab, coords, dist, av)
    for j, b in enumerate(ic.bands):
        ok, dev_ = tw.close(got["A_%s" % b].cpu().numpy(), w["sys_A"][j])
        assert ok, (b, dev_)
    # host arrays in, CUDA tensors out, the same values
    again = ia.evaluate_binaries(ic, mA, mB, age, feh, dist, av, eeps=None if eeps is None else (kw["eeps"], kw["eeps"]))
    for c in got:
        assert again[c].is_cuda and tw.same_bits(again[c].cpu().numpy(), got[c].cpu().numpy()), c


def _population(ic):
    from scipy.stats import uniform
    from isochrones_amd import populations as pp
    from isochrones_amd.priors import AVPrior, FlatPrior
    return pp.StarPopulation(ic, imf=FlatPrior((0.2, 1.2)), sfh=pp.StarFormationHistory(uniform(0.1, 0.25)),
                             feh=FlatPrior((-0.9, 0.4)), distance=FlatPrior((50.0, 500.0)), AV=AVPrior((0.0, 1.0)))


def test_generate_is_seeded_and_tensors_equal_the_frame():
    import torch
    pop = _population(tw.small_ic())
    df = pop.generate(300, seed=1)
    again = pop.generate(300, seed=1)
    assert len(df) == 300 and not df.mass_0.isnull().any() and df.equals(again)
    assert not pop.generate(300, seed=2).equals(df)
    d = pop.generate(300, seed=1, as_tensors=True)
    assert list(d) == list(df.columns)
    for c in df.columns:
        assert d[c].is_cuda and d[c].dtype == torch.float64
        assert tw.same_bits(d[c].cpu().numpy(), df[c].values), c
    exact = pop.generate(64, seed=3, accurate="exact", exact_N=False)
    assert 0 < len(exact) <= 64
    ok, dev_ = tw.close(exact["age_0"].values, exact["requested_age_0"].values)     # the exact solve hits the requested age
    assert ok, dev_
    from isochrones_amd import populations as pp
    dd = pp.deredden(d)
    frame = pp.deredden(df)
    for c in df.columns:
        assert tw.same_bits(dd[c].cpu().numpy(), frame[c].values), c


def test_golden_through_the_device_entry():
    from isochrones_amd import populations as pp
    tw.check_against_golden(tw.golden(), pp._DeviceBackend(0))


def test_isochrone_interpolator_delegates_to_its_track():
    import isochrones_amd as ia
    from isochrones_amd import models
    from oracle import make_golden as mg
    track = tw.small_ic()
    g, ax, names = mg.small_iso()
    grid = models.IsochroneGrid(ia.DFInterpolator.from_arrays(g, ax, names, ["log10_isochrone_age_yr", "feh", "EEP"]),
                                limits=mg.limits_of("iso", ax))
    iso = models.IsochroneInterpolator(grid, track.bc_grid, bands=track.bands, eep_bounds=(ax[2][0], ax[2][-1]))
    iso._companion_factory = lambda: track
    a, b = _population(iso).generate(100, seed=5), _population(track).generate(100, seed=5)
    assert a.equals(b) and len(a) == 100
