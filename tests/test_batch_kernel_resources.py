"""The two one-band single-star batch kernels - bench.py's kernel and its isochrone twin - run at six waves per SIMD without
scratch: the limits of single kernels in isochrones_amd/csrc/resources.py (KERNEL_LIMITS), which the build enforces next to
the families' scratch budgets."""
from isochrones_amd.csrc import build as B
from isochrones_amd.csrc import resources as R

SLIM = ("k_lnpost_fast<0, 1, 1, false, false>", "k_lnpost_fast<1, 1, 1, false, false>")


def test_one_band_batch_kernels_have_no_scratch_at_six_waves():
    B.build()
    t = B.resource_table()
    for k in SLIM:
        assert R.KERNEL_LIMITS[k] == {"scratch": 0, "vgpr": 80}
        assert t[k]["scratch"] == 0 and t[k]["vgpr"] <= 80 and t[k]["waves"] >= 6 and t[k]["agpr"] == 0, (k, t[k])


def test_a_kernel_over_its_own_limit_is_a_violation():
    t = {SLIM[0]: dict(sgpr=106, vgpr=80, agpr=0, scratch=12, waves=6, sgpr_spill=8, vgpr_spill=2, lds=0),
         SLIM[1]: dict(sgpr=106, vgpr=88, agpr=0, scratch=0, waves=5, sgpr_spill=8, vgpr_spill=0, lds=0)}
    bad = R.violations(t)
    assert len(bad) == 2 and "scratch = 12" in bad[0] and "vgpr = 88" in bad[1], bad
    # inside the family's budget alone both pass: the limits are the kernels' own
    assert R.violations(t, kernel_limits={}) == []
    t[SLIM[0]]["scratch"], t[SLIM[1]]["vgpr"] = 0, 80
    assert R.violations(t) == []
