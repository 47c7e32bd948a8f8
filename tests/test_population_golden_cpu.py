"""iso_population_eval_host against tests/golden/population/binary.npz - the reference's own
generate_binary(..., all_As=True) on the small synthetic tables (tools/make_population_golden.py): every column within 1e-9
(relative, with an absolute floor of 1e-9), the NaN pattern identical, the columns in the reference's order."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_harness
from tests import _population_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = tw.GOLDEN


def test_host_entry_reproduces_the_reference():
    from isochrones_amd import populations as pp
    g = tw.golden()
    assert g["values"].shape == (200, len(g["columns"])) and os.path.getsize(GOLDEN) < 263 * 1024
    worst = tw.check_against_golden(g, pp._HostBackend())
    print("largest deviation from the reference: %.3g" % worst)


def test_golden_holds_the_cases_it_was_drawn_for():
    g = tw.golden()
    cols = [str(c) for c in g["columns"]]
    v = g["values"]
    bands = [c[:-4] for c in cols if c.endswith("_mag")]
    assert len(bands) == 7 and len(cols) == 2 * (18 + 7 + 4 + 7) + 14
    sys_mags = v[:, [cols.index(b + "_mag") for b in bands]]
    sec = v[:, [cols.index(b + "_mag_1") for b in bands]]
    assert np.isnan(sys_mags).any(axis=1).mean() <= 0.40
    assert ((g["mass_B"] > 0) & np.isfinite(sec).all(axis=1) & np.isfinite(sys_mags).all(axis=1)).mean() >= 0.30
    assert (g["mass_B"] == 0).sum() >= 5 and np.isnan(v[:, cols.index("mass_0")]).sum() >= 5
    assert (g["AV"] == 0).sum() >= 5 and (g["AV"] == 1.0).sum() >= 5
    # an absent secondary leaves the primary's light; filled columns are filled for it too
    absent = g["mass_B"] == 0
    ok, dev = tw.close(v[absent][:, cols.index("V_mag")], v[absent][:, cols.index("V_mag_0")])
    assert ok, dev
    assert not np.isnan(v[absent][:, [cols.index(c) for c in ("distance_1", "AV_1", "initial_feh_1", "requested_age_1")]]).any()
    # the twin of the header agrees with the reference as well
    tab = tw.tables()
    from oracle import make_golden as mg
    gr, ax, names = mg.small_track()
    hot = tuple(list(names).index(n) for n in ("Teff", "logg", "feh", "Mbol"))
    tab = (np.ascontiguousarray(gr), tab[1], hot, tab[3], tab[4])
    coords = np.array([[g["feh"], g["mass_A"], g["eep_A"]], [g["feh"], g["mass_B"], g["eep_B"]]])
    w = tw.evaluate(tab, coords, g["distance"], g["AV"])
    for j, b in enumerate(bands):
        for key, col in (("sys_mag", b + "_mag"), ("sys_A", "A_" + b)):
            ok, dev = tw.close(w[key][j], v[:, cols.index(col)])
            assert ok, (col, dev)


@pytest.mark.skipif(os.environ.get("ISO_CHECK_GOLDENS") == "0" or not ref_harness.reference_available(),
                    reason="needs a checkout of the reference ($ISO_REFERENCE_ROOT)")
def test_population_fixture_regenerates_byte_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="12345")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_population_golden.py"), str(tmp_path)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["binary.npz"]
    assert filecmp.cmp(str(tmp_path / "binary.npz"), GOLDEN, shallow=False)
