"""libiso_reweight.so (the population-informed posterior of every star from its stored chain) builds for gfx950 without a
GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.REWEIGHT, its waves per
SIMD, a clean isa_check scan.  The library joins the build through libraries.NEWER; hier and select stay what they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries
from isochrones_amd.csrc.libraries import REWEIGHT as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.HIER.FLAGS == libraries.SELECT.FLAGS
    assert os.path.basename(_built()) == "libiso_reweight.so"
    assert [os.path.basename(s) for s in B.sources()] == ["reweight.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(os.path.normpath(path)).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path                  # every sum in a fixed order
    src = open(B.sources()[0]).read()
    assert '#include "../common/family_lnf.h"' in src and "feh_shape" not in src     # the family arithmetic is the shared one


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _hier_cabi as hc, _reweight_cabi as rc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_reweight.h")).read()
    assert '#include "isochrones_amd_hier.h"' in text
    syms = set(re.findall(r"\b(iso_reweight_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(rc.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(rc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_REWEIGHT_(\w+) (\S+)", text))
    assert int(consts["MAX_VALUES"]) == rc.MAX_VALUES == 8 and int(consts["MAX_PROBS"]) == rc.MAX_PROBS == 8
    assert int(consts["ROW_TILE"]) == rc.ROW_TILE
    assert int(consts["ERR_INVALID"].strip("()")) == rc.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == rc.ERR_HIP
    # the records and the column descriptors are the hierarchical library's, as they are: the header defines none
    assert rc.RECORD is hc.RECORD and rc.IsoHierColumn is hc.IsoHierColumn and rc.MAX_COLS == hc.MAX_COLS == 4
    assert not re.search(r"typedef struct", text.split("#ifndef")[1])
    assert os.path.samefile(path, rc.library_path())
    assert rc.EXPORTED_SYMBOLS[:2] == ("iso_reweight_version", "iso_reweight_last_error")
    lib.iso_reweight_version.restype = ctypes.c_char_p
    assert lib.iso_reweight_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_reweight_weights", "k_reweight_summary"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
    # max_vgpr is the occupancy step the weights kernel compiles to: 512 registers a SIMD lane, in granules of 8; more
    # waves than k_hier_stars's 3, since the rows' accumulators are gone.  A tile of rows in LDS leaves room for that
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_reweight_weights"]["waves"] == B.MIN_WAVES > libraries.HIER.MIN_WAVES
    assert table["k_reweight_weights"]["lds"] * 8 <= 160 * 1024 and table["k_reweight_summary"]["lds"] * 4 <= 160 * 1024
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.NEWER and B.name == "reweight" and libraries.SELECT in libraries.NEWER
    every = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert len({s.name for s in every}) == len(every)
    for a, b in itertools.combinations((main,) + every, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in every}) == len(every)
    assert not any("reweight" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_reweight.h", "isochrones_amd_hier.h", "family_lnf.h",
                                                          "grid_cell.h", "last_error.h", "wave_reduce.h", "hier_columns.h",
                                                          "chain_view.h"]
    # what build() and the command line iterate, and what git ignores
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER" in entry
    assert "isochrones_amd/csrc/libiso_reweight.resources.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
