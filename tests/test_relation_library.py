"""libiso_relation.so (the population likelihood for a density that links one column to another) builds for gfx950 without
a GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.RELATION, its waves
per SIMD, a clean isa_check scan.  The library joins the build through libraries.NEWER; hier, select and reweight stay what
they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries
from isochrones_amd.csrc.libraries import RELATION as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.HIER.FLAGS == libraries.SELECT.FLAGS == libraries.REWEIGHT.FLAGS
    assert os.path.basename(_built()) == "libiso_relation.so"
    assert [os.path.basename(s) for s in B.sources()] == ["relation.hip"]
    common = os.path.join(os.path.dirname(libraries.__file__), "common")
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path                  # every sum in a fixed order
    src = open(B.sources()[0]).read()
    # the kinds 1 .. 8 are the shared arithmetic, the linked one lives in a header SELECT and REWEIGHT can adopt
    assert '#include "../common/relation_lnf.h"' in src and "feh_shape" not in src
    rel = open(os.path.join(common, "relation_lnf.h")).read()
    assert '#include "family_lnf.h"' in rel and rel.count("erfc(") == 2 and "feh_shape" not in rel


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _hier_cabi as hc, _relation_cabi as rc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_relation.h")).read()
    assert '#include "isochrones_amd_hier.h"' in text
    syms = set(re.findall(r"\b(iso_relation_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(rc.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(rc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_RELATION_(\w+) (\S+)", text))
    assert int(consts["LINGAUSS"]) == rc.LINGAUSS == 9 and rc.LINGAUSS == hc.TRUNCGAUSS + 1
    assert int(consts["ROW_TILE"]) == rc.ROW_TILE
    assert int(consts["ERR_INVALID"].strip("()")) == rc.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == rc.ERR_HIP
    # the records and the column descriptors are the hierarchical library's, as they are: the header defines none
    assert rc.RECORD is hc.RECORD and rc.IsoHierColumn is hc.IsoHierColumn and rc.MAX_COLS == hc.MAX_COLS == 4
    assert not re.search(r"typedef struct", text.split("#ifndef")[1])
    # the likelihood entries take iso_hier_lnlike's argument list
    hier = open(os.path.join(ROOT, "include", "isochrones_amd_hier.h")).read()
    args = lambda t, name: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, t, re.S).group(1))
    for a, b in (("iso_relation_lnlike", "iso_hier_lnlike"), ("iso_relation_lnlike_host", "iso_hier_lnlike_host")):
        assert args(text, a) == args(hier, b)
    assert os.path.samefile(path, rc.library_path())
    assert rc.EXPORTED_SYMBOLS[:2] == ("iso_relation_version", "iso_relation_last_error")
    lib.iso_relation_version.restype = ctypes.c_char_p
    assert lib.iso_relation_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_relation_stars", "k_relation_total"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
    # max_vgpr is the occupancy step the stars kernel compiles to: 512 registers a SIMD lane, in granules of 8
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_relation_stars"]["waves"] == B.MIN_WAVES
    # the sample's values stay in registers: nothing per lane in LDS, which holds the tile's records and the reduction only
    assert table["k_relation_stars"]["lds"] <= 4096 and table["k_relation_total"]["lds"] <= 64
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.NEWER and B.name == "relation"
    assert libraries.SELECT in libraries.NEWER and libraries.REWEIGHT in libraries.NEWER
    every = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert len({s.name for s in every}) == len(every)
    for a, b in itertools.combinations((main,) + every, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in every}) == len(every)
    assert not any("relation" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == [
        "isochrones_amd_relation.h", "isochrones_amd_hier.h", "family_lnf.h", "grid_cell.h", "last_error.h", "wave_reduce.h",
        "relation_lnf.h", "hier_columns.h", "chain_view.h", "hier_block.h", "hier_lnlike.h"]
    # what build() and the command line iterate, and what git ignores
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER" in entry
    assert "isochrones_amd/csrc/libiso_relation.resources.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
