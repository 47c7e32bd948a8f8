"""Wherever a checkout of the reference is present: rerun tools/make_solve_golden.py - the reference's own
get_eep_accurate - into a scratch directory and require byte-identical fixtures (ISO_CHECK_GOLDENS=0 skips it, as the
pin of tests/golden/ itself)."""
import filecmp
import os
import subprocess
import sys

import pytest

from oracle import ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(os.environ.get("ISO_CHECK_GOLDENS") == "0" or not ref_harness.reference_available(),
                    reason="needs a checkout of the reference ($ISO_REFERENCE_ROOT)")
def test_solve_fixtures_regenerate_byte_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="12345")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_solve_golden.py"), str(tmp_path)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    kept_dir = os.path.join(ROOT, "tests", "golden", "solve")
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    kept = sorted(f for f in os.listdir(kept_dir) if f.endswith(".npz"))
    assert made == kept == ["iso.npz", "track.npz"]
    match, mismatch, errors = filecmp.cmpfiles(str(tmp_path), kept_dir, made, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
