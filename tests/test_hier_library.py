"""libiso_hier.so (the hierarchical population likelihood from the stored chains of a catalog) builds for gfx950 without a
GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.HIER, its waves per
SIMD, a clean isa_check scan.  The library joins the build through libraries.ADDED; BUILD_ORDER stays what it was."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries
from isochrones_amd.csrc.libraries import HIER as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert os.path.basename(_built()) == "libiso_hier.so"
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path          # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path              # L is summed in a fixed order
    src = open(os.path.join(B.SRC, "hier.hip")).read()
    assert '#include "../common/family_lnf.h"' in src and "feh_shape" not in src     # the family arithmetic is the shared one


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _hier_cabi as hc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_hier.h")).read()
    syms = set(re.findall(r"\b(iso_hier_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(hc.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(hc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_HIER_(\w+) (\S+)", text))
    assert int(consts["MAX_COLS"]) == hc.MAX_COLS == 4 and int(consts["NPAR"]) == hc.NPAR == 6
    assert int(consts["ROW_TILE"]) == hc.ROW_TILE == 8
    assert int(consts["ERR_INVALID"].strip("()")) == hc.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == hc.ERR_HIP
    for name in ("FLAT", "FLATLOG", "POWERLAW", "GAUSS", "LOGNORMAL", "CHABRIER", "FEH", "TRUNCGAUSS"):
        assert int(consts[name]) == getattr(hc, name)
    from isochrones_amd import _cabi
    assert (hc.FLAT, hc.FLATLOG, hc.POWERLAW, hc.GAUSS, hc.LOGNORMAL, hc.CHABRIER, hc.FEH) == (
        _cabi.PRIOR_FLAT, _cabi.PRIOR_FLATLOG, _cabi.PRIOR_POWERLAW, _cabi.PRIOR_GAUSS, _cabi.PRIOR_LOGNORMAL,
        _cabi.PRIOR_CHABRIER, _cabi.PRIOR_FEH)
    assert hc.RECORD.itemsize == 72 and hc.RECORD.fields["lo"][1] == 8 and hc.RECORD.fields["p"][1] == 24
    assert ctypes.sizeof(hc.IsoHierColumn) == 24
    assert np.dtype(hc.RECORD).isalignedstruct
    assert os.path.samefile(path, hc.library_path())
    assert hc.EXPORTED_SYMBOLS[:2] == ("iso_hier_version", "iso_hier_last_error")
    lib.iso_hier_version.restype = ctypes.c_char_p
    assert lib.iso_hier_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_hier_stars", "k_hier_total"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
    # max_vgpr is the occupancy step the kernel compiles to: 512 registers a SIMD lane, in granules of 8
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_hier_stars"]["waves"] == B.MIN_WAVES
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert [s.name for s in libraries.BUILD_ORDER] == ["cluster", "nested", "solve", "diag", "derived", "predict", "population"]
    assert libraries.ADDED == (B,) and B.name == "hier"
    every = libraries.BUILD_ORDER + libraries.ADDED
    for a, b in itertools.combinations((main,) + every, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in every}) == len(every)
    assert not any("hier" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == [
        "isochrones_amd_hier.h", "family_lnf.h", "grid_cell.h", "last_error.h", "wave_reduce.h", "hier_columns.h", "chain_view.h",
        "hier_block.h", "hier_lnlike.h"]
    # what build() iterates, and what git ignores
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED" in entry
    assert "isochrones_amd/csrc/libiso_hier.resources.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
