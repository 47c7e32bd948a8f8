"""libiso_members.so on the device through its C ABI: against the long-double twin (tests/_members_twin.py) and against the host
entry at 1e-11 (1 + |x|), with ln_like the same bits as lnlike_star of iso_cluster_lnlike on every case.

Synthetic ABI inputs from a seeded generator go straight to iso_members_moments: there is no interpolation in the loop, so a
failure points at the kernels.  The shapes sit at the seams: 63 / 64 / 65 / 130 stars (the pairs kernel's tile of 64), ld 64 /
65 / 66 / 129 / 130 (secondaries in blocks of 64), n_valid in {0, 1, 2, ld - 3, ld}, 1 / 3 / 32 bands (32: the launch that
asks for more than 64 KB of LDS), 0 / 8 properties, fB of 0 and 1, minq 0.9, a star whose every cell underflows.  Every
output lies between margins that have to come back untouched."""
import numpy as np
import pytest

from isochrones_amd import device as dev

from . import _members_twin as mt

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def lib():
    from isochrones_amd import _members_cabi as mc
    return mc.lib()


@pytest.fixture(scope="module")
def cuda():
    import torch
    return torch.device("cuda", 0)


def cluster_star_terms(a, device, rows=None):
    """lnlike_star [P, N_s] of iso_cluster_lnlike on the same inputs."""
    import torch
    from isochrones_amd import _cluster_cabi as CC
    rows = np.arange(a["n_valid"].size) if rows is None else np.asarray(rows)
    P, ns, ld = rows.size, a["ns"], a["ld"]
    t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=device)   # noqa: E731
    cols, nv, rp = t(a["cols"][rows]), t(a["n_valid"][rows], torch.int32), t(a["rowpar"][rows])
    val, w = t(a["star_val"]), t(a["star_w"])
    work = torch.empty(P * ns * ld, dtype=torch.float64, device=device)
    tot = torch.empty(P, dtype=torch.float64, device=device)
    per_star = torch.full((P, ns), mt.FILL, dtype=torch.float64, device=device)
    CC.check(CC.lib().iso_cluster_lnlike(dev.ptr(cols), ld, P, dev.ptr(nv), dev.ptr(rp), dev.ptr(val), dev.ptr(w), ns, a["nb"],
                                         a["npr"], a["minq"], dev.ptr(work), dev.ptr(tot), dev.ptr(per_star),
                                         dev.stream_ptr(device.index)))
    torch.cuda.synchronize(device)
    return per_star.cpu().numpy()


def test_the_list_covers_the_seams():
    cs = [mt.CASES[n] for n in mt.GPU_CASES]
    assert {63, 64, 65, 130} <= {c["ns"] for c in cs} and {64, 65, 66, 129, 130} <= {c["ld"] for c in cs}
    assert {1, 3, 32} <= {c["nb"] for c in cs} and {0, 8} <= {c["npr"] for c in cs}
    assert {0.0, 1.0, None} <= {c.get("fB") for c in cs} and {0.1, 0.9} <= {c.get("minq", 0.1) for c in cs}
    assert any(c.get("off") for c in cs)
    assert max(c["ld"] for c in cs if c["nb"] == 32) > 64               # a second block of secondaries on the big-LDS path
    assert (4 * 32 + 3) * 64 * 8 + 64 * 4 > 64 * 1024 >= (4 * 31 + 3) * 64 * 8 + 64 * 4


@pytest.mark.parametrize("name", mt.GPU_CASES)
def test_device_matches_the_twin_the_host_entry_and_the_likelihood(lib, cuda, name):
    a, (ln, mom) = mt.case(name)
    rc, got_ln, got_mom, _ = mt.call(lib, a, device=cuda)
    assert rc == 0, lib.iso_members_last_error()
    e1 = mt.close(got_ln, ln, "ln_like vs twin", WORST)
    e2 = mt.close(got_mom, mom, "moments vs twin", WORST)
    rc, host_ln, host_mom, _ = mt.call(lib, a)
    assert rc == 0
    e3 = mt.close(got_ln, host_ln, "ln_like vs host", WORST)
    e4 = mt.close(got_mom, host_mom, "moments vs host", WORST)
    print("%-30s worst |d| / (1 + |ref|): twin %.2e %.2e, host %.2e %.2e" % (name, e1, e2, e3, e4))
    assert mt.same_bits(got_ln, cluster_star_terms(a, cuda)), "ln_like is not lnlike_star of iso_cluster_lnlike bit for bit"
    dead = np.isneginf(got_ln)
    assert np.isnan(got_mom[dead]).all() and not np.isnan(got_mom[~dead]).any() and not np.isnan(got_ln).any()
    if name == "underflow_star":
        assert dead[3:, 10].all() and not dead[3:, :10].any() and not dead[3:, 11:].any()
    if mt.CASES[name].get("fB") == 0.0:
        assert np.all(got_mom[~dead][:, 8] == 0.0) and np.all(got_mom[~dead][:, 9] == 1.0)
    if mt.CASES[name].get("fB") == 1.0:
        assert np.all(got_mom[~dead][:, 8] == 1.0) and np.all(got_mom[~dead][:, 9] == 0.0)
    if mt.CASES[name]["nb"] == 1:
        assert np.all(np.abs(got_mom[~dead][:, 8] + got_mom[~dead][:, 9] - 1.0) <= 1e-12)


def test_the_constructed_case_on_the_device(lib, cuda):
    a = mt.constructed()
    rc, ln, mom, _ = mt.call(lib, a, device=cuda)
    assert rc == 0
    assert mom[0, 0, 9] > 0.99 and mom[0, 1, 8] > 0.9 and 1.2 < mom[0, 1, 2] < 1.45
    ref_ln, ref_mom = mt.reference(a)
    mt.close(ln, ref_ln, "ln_like vs twin", WORST)
    mt.close(mom, ref_mom, "moments vs twin", WORST)
    assert mt.same_bits(ln, cluster_star_terms(a, cuda))


def test_a_row_is_the_same_bits_in_any_company(lib, cuda):
    """Alone, in a batch of 7, reversed, in chunks of 3 and on a repeated call."""
    a, _ = mt.case("64stars_ld65_8props")
    seven = [4, 3, 2, 4, 0, 1, 3]
    rc, ln, mom, _ = mt.call(lib, a, device=cuda, rows=seven)
    assert rc == 0
    rc, ln2, mom2, _ = mt.call(lib, a, device=cuda, rows=seven)
    assert rc == 0 and mt.same_bits(ln, ln2) and mt.same_bits(mom, mom2)
    rc, lr, mr, _ = mt.call(lib, a, device=cuda, rows=seven[::-1])
    assert rc == 0 and mt.same_bits(lr[::-1], ln) and mt.same_bits(mr[::-1], mom)
    for c0 in range(0, 7, 3):
        rc, lc, mcn, _ = mt.call(lib, a, device=cuda, rows=seven[c0:c0 + 3])
        assert rc == 0 and mt.same_bits(lc, ln[c0:c0 + 3]) and mt.same_bits(mcn, mom[c0:c0 + 3])
    for i, r in enumerate(seven):
        rc, l1, m1, _ = mt.call(lib, a, device=cuda, rows=[r])
        assert rc == 0 and mt.same_bits(l1[0], ln[i]) and mt.same_bits(m1[0], mom[i]), (i, r)
    assert mt.same_bits(ln[0], ln[3]) and mt.same_bits(mom[1], mom[6])          # the same row twice in one launch


def test_nothing_is_written_past_n_valid(lib, cuda):
    a, _ = mt.case("63stars_ld64_1band")
    rc, _, _, work = mt.call(lib, a, device=cuda)
    assert rc == 0
    for r, n in enumerate(np.clip(a["n_valid"], 0, a["ld"])):
        assert np.all(work[r][:, :, n:] == mt.FILL) and not np.any(work[r][:, :, :n] == mt.FILL), r


def test_a_side_stream_gives_the_same_bits(lib, cuda):
    import torch
    a, _ = mt.case("130stars_ld129")
    rc, ln, mom, _ = mt.call(lib, a, device=cuda)
    side = torch.cuda.Stream(device=cuda)
    rc2, ln2, mom2, _ = mt.call(lib, a, device=cuda, stream=side)
    assert rc == 0 and rc2 == 0 and mt.same_bits(ln, ln2) and mt.same_bits(mom, mom2)


@pytest.mark.parametrize("over, word", [(dict(n_bands=0), "bands"), (dict(n_bands=33), "bands"), (dict(n_props=9), "props"),
                                        (dict(cols=None), "null"), (dict(moments=None), "null")])
def test_refused_shapes_launch_nothing(lib, cuda, over, word):
    from isochrones_amd import _members_cabi as mc
    a, _ = mt.case("63stars_ld64_1band")
    rc, ln, mom, work = mt.call(lib, a, device=cuda, **over)
    assert rc == mc.ERR_INVALID
    msg = lib.iso_members_last_error().decode()
    assert "iso_members_moments" in msg and word in msg
    assert np.all(ln == mt.FILL) and np.all(mom == mt.FILL) and np.all(work == mt.FILL)


def test_zz_worst_error():
    """(last) the largest differences of this module's comparisons"""
    print("worst |got - ref| / (1 + |ref|): " + ", ".join("%s %.3e" % kv for kv in sorted(WORST.items())))
    assert max(WORST.values(), default=0.0) <= mt.TOL
