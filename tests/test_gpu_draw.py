"""iso_draw_systems (k_draw_systems) on the device against iso_draw_systems_host on the same records: every kind within 1e-11,
every discrete choice (TABLE bin, Chabrier piece, FEH component) equal, a LINGAUSS window without mass at the near bound;
N = 1, 63, 64, 65 (a wavefront and its neighbours), 257 (a second workgroup) and 4 099; C = 1 and 8; first = 2^32 - 3 (the counter's high word); a shuffled index; the rounds;
bit identity of a column alone and among eight, of a repeated call and of a call on another stream; N = CAP + 257 and
2 * CAP + 1 with CAP = ISO_DRAW_MAX_BLOCKS * 256 (the second and the third trip of the stride loop).  No test here is
statistical: the host entry is held to the distributions on the CPU."""
import numpy as np
import pytest

from isochrones_amd import _draw_cabi as dc, draws, priors as P
from tests import _draw_twin as tw

pytestmark = pytest.mark.gpu
WORST = [0.0]


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def on_device(plan, n, seed, device, rnd=0, first=0, index=None):
    out = plan.draw(n, seed, round=rnd, first=first, index=index, device=device)
    import torch
    torch.cuda.synchronize(device)
    return np.stack([out[name].cpu().numpy() for name in plan.device_columns])


def choices(plan, x):
    """The discrete choice behind every value of the columns that have one: the TABLE bin, the Chabrier piece (which side of
    the breakpoint), the FEH component (recovered by the twin from the same uniforms: the thresholds are the record's)."""
    out = {}
    for q, name in enumerate(plan.device_columns):
        R = plan.records[q]
        if int(R["kind"]) == dc.TABLE:
            e = plan.specs[name].table[0]
            out[name] = np.clip(np.searchsorted(e, x[q], side="right") - 1, 0, e.size - 2)
        elif int(R["kind"]) == dc.CHABRIER:
            out[name] = x[q] >= plan.specs[name].breakpoint
    return out


def against_host(plan, got, seed, rnd, first, what):
    """``got`` [C, n], the device's systems first .. first + n - 1, against the host entry on the same global numbers:
    finite, inside the records' bounds, within tw.TOL, every discrete choice equal."""
    n = got.shape[1]
    ref = tw.host(plan, n, seed, rnd, first)
    assert np.all(np.isfinite(got))
    assert np.all((got >= plan.records["lo"][:, None]) & (got <= plan.records["hi"][:, None]))
    worst = tw.error(plan, got, ref.astype(np.longdouble))
    WORST[0] = max(WORST[0], worst)
    print("device against the host entry, %s, N = %d, round %d: %.3g" % (what, n, rnd, worst))
    assert worst < tw.TOL
    a, b = choices(plan, got), choices(plan, ref)
    for col in a:
        assert np.array_equal(a[col], b[col]), col
    # the FEH component of every value, named from the value itself, equals the host entry's and the one the record's
    # thresholds give for u0
    for q, col in enumerate(plan.device_columns):
        R = plan.records[q]
        if int(R["kind"]) == dc.FEH:
            j = first + np.arange(n, dtype=np.int64)
            u = tw.uniforms(seed, j, int(R["stream"]), rnd)
            want = np.where(u[:, 0] < R["p"][1], 0, np.where(u[:, 0] < R["p"][2], 1, 2))
            assert np.array_equal(tw.feh_component(R, u[:, 1], got[q]), want), col
            assert np.array_equal(tw.feh_component(R, u[:, 1], ref[q]), want), col


@pytest.mark.parametrize("name", sorted(tw.PLANS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_device_matches_the_host_entry(device, name, n):
    plan = draws.DrawPlan(tw.PLANS[name]())
    assert len(plan.records) == (5 if name == "far" else 8)
    for rnd, first in ((0, 0), (1, 2 ** 32 - 3)):
        against_host(plan, on_device(plan, n, 42, device, rnd, first), 42, rnd, first, name)
    # the rounds differ
    assert not np.array_equal(on_device(plan, n, 42, device, 0, 0)[0], on_device(plan, n, 42, device, 1, 0)[0])


def test_one_column(device):
    for n in (1, 65, 4099):
        plan = draws.DrawPlan({"x": P.ChabrierPrior()})
        got, ref = on_device(plan, n, 5, device), tw.host(plan, n, 5)
        assert tw.error(plan, got, ref.astype(np.longdouble)) < tw.TOL
        assert np.array_equal(got[0] >= 1.0, ref[0] >= 1.0)


def test_bit_identity(device):
    import torch
    cols = tw.every_kind()
    plan = draws.DrawPlan(cols)
    n = 4099
    first = 2 ** 32 - 3
    full = on_device(plan, n, 9, device, 1, first)
    assert np.array_equal(full, on_device(plan, n, 9, device, 1, first))           # a repeated call
    for q, name in enumerate(plan.device_columns):                                   # a column alone against among eight
        alone = draws.DrawPlan({name: cols[name]}, streams={name: q})
        assert np.array_equal(on_device(alone, n, 9, device, 1, first)[0], full[q]), name
    # a sub-range through first, the same systems through a shuffled index
    sub = on_device(plan, 300, 9, device, 1, first + 1000)
    assert np.array_equal(sub, full[:, 1000:1300])
    perm = np.random.default_rng(0).permutation(300)
    assert np.array_equal(on_device(plan, 300, 9, device, 1, 0, index=first + 1000 + perm), sub[:, perm])
    # linked columns: the parent comes from a register, the child is the same bits wherever the system stands
    link = draws.DrawPlan(tw.linked())
    lf = on_device(link, 257, 9, device, 0, first)
    back = on_device(link, 257, 9, device, 0, 0, index=torch.arange(first + 256, first - 1, -1, device=device))
    assert np.array_equal(back[:, ::-1], lf)
    # a call on a non-default stream
    stream = torch.cuda.Stream(device)
    with torch.cuda.stream(stream):
        other = plan.draw(n, 9, round=1, first=first, device=device)
    stream.synchronize()
    assert np.array_equal(np.stack([other[c].cpu().numpy() for c in plan.device_columns]), full)


# ---- beyond the grid's cap: the second and the third trip of the kernel's stride loop ------------------------------------------

BLOCK = 256                                                          # lanes of a workgroup
CAP = dc.MAX_BLOCKS * BLOCK                                          # systems of one trip of the capped grid
MARGIN = 64
BIG_FIRST, BIG_ROUND, BIG_SEED = 2 ** 32 - 3, 1, 42


def raw_draw(plan, n, device, first=BIG_FIRST, index=None):
    """iso_draw_systems into a [C, n] buffer of NaN (no draw is one) between two margins of NaN, which have to stay so.
    Returns the device tensor: every value finite, so no NaN is left in the range the kernel has to write."""
    import torch
    from isochrones_amd import device as dev
    C_ = len(plan.records)
    flat = torch.full((C_ * n + 2 * MARGIN,), float("nan"), dtype=torch.float64, device=device)
    x = flat[MARGIN:MARGIN + C_ * n].view(C_, n)
    tb = torch.from_numpy(plan.tables).to(device) if plan.tables.size else None
    with torch.cuda.device(device):
        dc.check(dc.lib().iso_draw_systems(plan.records.ctypes.data, C_, plan.order.ctypes.data, dev.ptr(tb), plan.tables.size,
                                           BIG_SEED, BIG_ROUND, int(first), dev.ptr(index), n, dev.ptr(x),
                                           dev.stream_ptr(device.index)))
    torch.cuda.synchronize(device)
    assert bool(torch.isnan(flat[:MARGIN]).all()) and bool(torch.isnan(flat[-MARGIN:]).all()), "a write outside x"
    assert bool(torch.isfinite(x).all()), "a system was not written"
    lo, hi = (torch.from_numpy(np.ascontiguousarray(plan.records[k])).to(device)[:, None] for k in ("lo", "hi"))
    assert bool(((x >= lo) & (x <= hi)).all())
    return x


@pytest.fixture(scope="module")
def beyond_the_cap(device):
    """{plan: (DrawPlan, x [C, CAP + 257] on the device)}: one lane in 4096 * 256 takes a second system; drawn once."""
    out = {}
    for name in ("kinds", "linked"):
        plan = draws.DrawPlan(tw.PLANS[name]())
        out[name] = (plan, raw_draw(plan, CAP + BLOCK + 1, device))
    yield out
    out.clear()


@pytest.mark.parametrize("name", ["kinds", "linked"])
def test_a_second_trip_of_the_stride_loop(device, beyond_the_cap, name):
    """N = CAP + 257, CAP = ISO_DRAW_MAX_BLOCKS * 256: the first 257 lanes of the grid draw a second system.  The result is
    the call of exactly CAP systems followed by the call of the other 257, bit for bit (compared on the device); around
    both ends of the first trip it is the host entry's."""
    import torch
    plan, x = beyond_the_cap[name]
    n = CAP + BLOCK + 1
    assert dc.MAX_BLOCKS == 4096 and x.shape == (8, n) and BIG_FIRST + 3 == 2 ** 32      # the counter's high word changes
    assert torch.equal(x[:, :CAP], raw_draw(plan, CAP, device))
    assert torch.equal(x[:, CAP:], raw_draw(plan, BLOCK + 1, device, first=BIG_FIRST + CAP))
    for a, b in ((0, 300), (CAP - 150, n)):
        against_host(plan, x[:, a:b].cpu().numpy(), BIG_SEED, BIG_ROUND, BIG_FIRST + a, "%s [%d, %d)" % (name, a, b))


@pytest.mark.parametrize("name", ["kinds", "linked"])
def test_the_second_trip_reads_the_index(device, beyond_the_cap, name):
    """The same systems through ``index``, the global numbers reversed (and ``first`` another number): the reversed result."""
    import torch
    plan, x = beyond_the_cap[name]
    n = CAP + BLOCK + 1
    index = torch.arange(BIG_FIRST + n - 1, BIG_FIRST - 1, -1, dtype=torch.int64, device=device)
    assert index.shape == (n,) and int(index[-1]) == BIG_FIRST
    assert torch.equal(raw_draw(plan, n, device, first=5, index=index).flip(1), x)


def test_a_third_trip_of_one_lane(device):
    """``linked`` at N = 2 * CAP + 1: lane 0 of workgroup 0 carries a parent and its table rows into a third system."""
    import torch
    plan = draws.DrawPlan(tw.linked())
    n = 2 * CAP + 1
    x = raw_draw(plan, n, device)
    tail = raw_draw(plan, BLOCK + 2, device, first=BIG_FIRST + n - (BLOCK + 2))
    assert torch.equal(x[:, n - (BLOCK + 2):], tail)
    against_host(plan, x[:, n - (BLOCK + 2):].cpu().numpy(), BIG_SEED, BIG_ROUND, BIG_FIRST + n - (BLOCK + 2), "linked, third trip")


def test_measured_maximum_is_reported():
    print("device against the host entry, maximum: %.3g" % WORST[0])
    assert WORST[0] < tw.TOL
