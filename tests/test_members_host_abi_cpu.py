"""libiso_members.so's host entry through ctypes, no GPU needed: iso_members_moments_host against the long-double twin of
tests/_members_twin.py at 1e-11 (1 + |x|) on ln_like and on every moment (the bound tests/test_gpu_cluster_abi.py holds the
likelihood to), over 1 / 65 / 130 stars, ld 5 / 66 / 130, n_valid in {0, 1, 2, ld - 3, ld}, 1 / 3 / 32 bands, 0 / 2 / 8
properties, fB of 0, 0.3 and 1, minq 0.1 and 0.9; a star whose every cell underflows; what one band, fB = 0 and fB = 1 make
exact; every refusal with its message; and a constructed case whose answer is known."""
import numpy as np
import pytest

from isochrones_amd import _members_cabi as mc
from isochrones_amd.csrc.libraries import MEMBERS
from tests import _members_twin as mt

WORST = {}


@pytest.fixture(scope="module")
def lib():
    MEMBERS.build()
    return mc.lib()


def _err(lib):
    return lib.iso_members_last_error().decode()


def test_the_list_covers_the_shapes():
    cs = [mt.CASES[n] for n in mt.HOST_CASES]
    assert {1, 65, 130} <= {c["ns"] for c in cs} and {5, 66, 130} <= {c["ld"] for c in cs}
    assert {1, 3, 32} <= {c["nb"] for c in cs} and {0, 2, 8} <= {c["npr"] for c in cs}
    assert {0.0, 1.0, None} <= {c.get("fB") for c in cs} and {0.1, 0.9} <= {c.get("minq", 0.1) for c in cs}
    assert all(c["ld"] <= 66 and c["ns"] <= 65 for c in cs if c["nb"] == 32)
    assert mt.rows_of(66) == [0, 1, 2, 63, 66]


@pytest.mark.parametrize("name", mt.HOST_CASES)
def test_host_entry_matches_the_twin(lib, name):
    a, (ln, mom) = mt.case(name)
    rc, got_ln, got_mom, _ = mt.call(lib, a)
    assert rc == 0, _err(lib)
    e1 = mt.close(got_ln, ln, "ln_like", WORST)
    e2 = mt.close(got_mom, mom, "moments", WORST)
    print("%-32s worst |d| / (1 + |ref|): ln_like %.2e, moments %.2e" % (name, e1, e2))
    dead = np.isneginf(got_ln)
    assert np.isnan(got_mom[dead]).all() and not np.isnan(got_mom[~dead]).any() and not np.isnan(got_ln).any()
    assert dead[:2].all() and np.isfinite(got_ln[-1]).sum() >= (a["ns"] + 1) // 2     # n_valid 0 and 1: no cell; ld: most stars


def test_a_star_50_mag_off_is_dead_and_alone_in_it(lib):
    a, (ln, mom) = mt.case("underflow_star")
    rc, got_ln, got_mom, _ = mt.call(lib, a, rows=[4])
    assert rc == 0
    assert got_ln[0, 10] == -np.inf and np.isnan(got_mom[0, 10]).all() and got_mom[0, 10].size == 11
    rest = np.delete(np.arange(a["ns"]), 10)
    assert np.isfinite(got_ln[0, rest]).all() and np.isfinite(got_mom[0, rest]).all()


def test_one_band_pair_and_single_share_everything(lib):
    for name in ("1star_ld5_1band", "minq09_1band"):
        a, _ = mt.case(name)
        rc, got_ln, got_mom, _ = mt.call(lib, a)
        live = np.isfinite(got_ln)
        assert rc == 0 and live.any()
        assert np.all(np.abs(got_mom[live][:, 8] + got_mom[live][:, 9] - 1.0) <= 1e-12), name
    a, _ = mt.case("130stars_ld130_3bands_8props")                      # three bands: the mixed states take the rest
    rc, got_ln, got_mom, _ = mt.call(lib, a, rows=[4])
    live = np.isfinite(got_ln)
    total = got_mom[live][:, 8] + got_mom[live][:, 9]
    assert np.all(total <= 1.0 + 1e-12) and np.any(total < 1.0 - 1e-6)


def test_fB_of_0_and_1_are_exact(lib):
    for name, pair, single in (("fB0", 0.0, 1.0), ("fB1", 1.0, 0.0)):
        a, _ = mt.case(name)
        rc, got_ln, got_mom, _ = mt.call(lib, a)
        live = np.isfinite(got_ln)
        assert rc == 0 and live.sum() > a["ns"]
        assert np.all(got_mom[live][:, 8] == pair) and np.all(got_mom[live][:, 9] == single), name
        assert np.isnan(got_mom[~live]).all() and not np.isnan(got_ln).any()
        if pair == 0.0:
            assert np.all(got_mom[live][:, 10] == 0.0)


def test_the_constructed_case_means_something(lib):
    """A float64 numpy prototype of the definition gives p_single 1.0000 for star A, p_pair 0.978 and a primary mass of 1.311
    for star B."""
    a = mt.constructed()
    rc, ln, mom, _ = mt.call(lib, a)
    assert rc == 0 and np.isfinite(ln).all() and np.isfinite(mom).all()
    print("star A: p_single %.4f; star B: p_pair %.4f, primary mass %.4f, q_pair %.4f"
          % (mom[0, 0, 9], mom[0, 1, 8], mom[0, 1, 2], mom[0, 1, 10] / mom[0, 1, 8]))
    assert mom[0, 0, 9] > 0.99
    assert mom[0, 1, 8] > 0.9
    assert 1.2 < mom[0, 1, 2] < 1.45
    ref_ln, ref_mom = mt.reference(a)
    mt.close(ln, ref_ln, "ln_like", WORST)
    mt.close(mom, ref_mom, "moments", WORST)


def test_rows_do_not_depend_on_their_batch(lib):
    a, _ = mt.case("64stars_ld65_8props")
    rc, ln, mom, work = mt.call(lib, a)
    assert rc == 0
    for r in (2, 4):
        rc, l1, m1, w1 = mt.call(lib, a, rows=[r])
        n = int(np.clip(a["n_valid"][r], 0, a["ld"]))
        assert rc == 0 and mt.same_bits(l1[0], ln[r]) and mt.same_bits(m1[0], mom[r])
        assert mt.same_bits(w1[0][:, :, :n], work[r][:, :, :n])
        assert np.all(w1[0][:, :, n:] == mt.FILL)                       # nothing is written past n_valid


@pytest.mark.parametrize("over, word", [(dict(n_bands=0), "bands"), (dict(n_bands=33), "bands"), (dict(n_props=9), "props"),
                                        (dict(n_props=-1), "props"), (dict(n_stars=0), "n_stars"), (dict(ld=0), "ld"),
                                        (dict(n_rows=-1), "n_rows"), (dict(cols=None), "null"), (dict(work=None), "null"),
                                        (dict(ln_like=None), "null"), (dict(moments=None), "null"),
                                        (dict(n_valid=None), "null")])
def test_refusals_have_a_message_and_write_nothing(lib, over, word):
    a, _ = mt.case("1star_ld5_1band")
    rc, ln, mom, work = mt.call(lib, a, **over)
    assert rc == mc.ERR_INVALID
    assert "iso_members_moments_host" in _err(lib) and word in _err(lib)
    assert np.all(ln == mt.FILL) and np.all(mom == mt.FILL) and np.all(work == mt.FILL)
    rc, _, _, _ = mt.call(lib, a)
    assert rc == 0 and _err(lib) == ""


def test_zz_worst_error():
    """(last) the largest error of this module's comparisons against the twin"""
    print("worst |got - ref| / (1 + |ref|): " + ", ".join("%s %.3e" % kv for kv in sorted(WORST.items())))
    assert max(WORST.values(), default=0.0) <= mt.TOL
