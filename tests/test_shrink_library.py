"""libiso_shrink.so (every star's weights and bin memberships under a binned population density) builds for gfx950 without a
GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.SHRINK, its waves per
SIMD, a clean isa_check scan.  The library joins the build through libraries.LATEST; the earlier tuples stay what they
were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries, sidelib
from isochrones_amd.csrc.libraries import SHRINK as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.HIER.FLAGS == libraries.BINNED.FLAGS == libraries.REWEIGHT.FLAGS
    assert os.path.basename(_built()) == "libiso_shrink.so"
    assert [os.path.basename(s) for s in B.sources()] == ["shrink.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path                  # every sum in a fixed order
    src = open(B.sources()[0]).read()
    # the kinds 1 .. 8, the wavefront reductions, the column view and the per-sample term are the shared headers'
    for shared in ("family_lnf.h", "chain_view.h", "hier_columns.h", "wave_reduce.h", "binned_sample.h"):
        assert '#include "../common/%s"' % shared in src
    for gone in ("__shfl_xor", "struct DevCol", "feh_shape", "thread_local", "struct Grid", "int bracket("):
        assert gone not in src, gone


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _binned_cabi as bc, _hier_cabi as hc, _shrink_cabi as sc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_shrink.h")).read()
    assert '#include "isochrones_amd_hier.h"' in text
    syms = set(re.findall(r"\b(iso_shrink_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(sc.EXPORTED_SYMBOLS) and len(syms) == 6
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(sc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_SHRINK_(\w+) (\S+)", text))
    assert int(consts["CELL_TILE"]) == sc.CELL_TILE
    assert int(consts["ERR_INVALID"].strip("()")) == sc.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == sc.ERR_HIP
    # the records and the column descriptors are the hierarchical library's, the grid's limits the binned library's, as
    # they are: the header defines no type and no limit of its own
    assert sc.RECORD is hc.RECORD and sc.IsoHierColumn is hc.IsoHierColumn and sc.MAX_COLS == hc.MAX_COLS == 4
    assert sc.MAX_CELLS == bc.MAX_CELLS and sc.MAX_AXES == bc.MAX_AXES and set(consts) == {"CELL_TILE", "ERR_INVALID", "ERR_HIP"}
    assert not re.search(r"typedef struct|\bstruct\b", text.split("#ifndef")[1])
    # a device entry and its host entry take the same arguments; the grid arguments are iso_binned_compress's, word for word
    args = lambda name, t=text: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, t, re.S).group(1))
    assert args("iso_shrink_cells") == args("iso_shrink_cells_host")
    assert args("iso_shrink_weights") == args("iso_shrink_weights_host")
    binned = args("iso_binned_compress", open(os.path.join(ROOT, "include", "isochrones_amd_binned.h")).read())
    upto = "const double* edges, "
    assert args("iso_shrink_weights").startswith(binned[:binned.index(upto) + len(upto)])
    assert "extra" not in args("iso_shrink_weights")
    assert os.path.samefile(path, sc.library_path())
    assert sc.EXPORTED_SYMBOLS[:2] == ("iso_shrink_version", "iso_shrink_last_error")
    lib.iso_shrink_version.restype = ctypes.c_char_p
    assert lib.iso_shrink_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_shrink_cells", "k_shrink_weights"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
        # nothing spills to memory.  The weights kernel's argument block overflows the SGPR file into VGPR lanes, as
        # k_binned_compress's (24) does: pinned, so that growth is noticed
        assert r["sgpr_spill"] <= (10 if name == "k_shrink_weights" else 0), (name, r)
    # max_vgpr is the occupancy step the weights kernel compiles to: 512 registers a SIMD lane, in granules of 8
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_shrink_weights"]["waves"] == B.MIN_WAVES
    assert B.MIN_WAVES == libraries.BINNED.MIN_WAVES                 # k_binned_compress's per-sample work, its occupancy
    # the cells kernel keeps the full occupancy: 64 registers, and LDS for ten workgroups a CU
    assert table["k_shrink_cells"]["waves"] == 8 and table["k_shrink_cells"]["vgpr"] <= 64
    # LDS: the records, the edges and the star's lnG; a tile's maxima and sums of 256 stars
    assert table["k_shrink_weights"]["lds"] <= 2048 and table["k_shrink_cells"]["lds"] <= 16384
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.LATEST and B.name == "shrink"
    assert B not in libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert [s.name for s in libraries.NEWER] == ["select", "reweight", "relation", "binned"]
    assert len({s.name for s in EVERY}) == len(EVERY)
    for a, b in itertools.combinations((main,) + EVERY, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in EVERY}) == len(EVERY)
    assert not any("shrink" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_shrink.h", "isochrones_amd_binned.h",
                                                          "isochrones_amd_hier.h", "family_lnf.h", "grid_cell.h", "last_error.h",
                                                          "wave_reduce.h", "hier_columns.h", "chain_view.h", "binned_sample.h"]
    # what build() and the command line iterate, and what git ignores
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST" in entry
    lines = open(os.path.join(ROOT, "isochrones_amd", "csrc", "libraries.py")).read()
    assert "for spec in BUILD_ORDER + ADDED + NEWER + LATEST}" in lines
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "isochrones_amd/csrc/libiso_shrink.resources.json" in ignored and "*.stamp" in ignored


def test_the_digest_covers_every_header_the_sources_reach():
    """A header that is reached but not listed would not rebuild the library when it is edited (the walk of
    tests/test_side_libraries_cpu.py, which is parametrised over the earlier tuples)."""
    followed = {os.path.realpath(d) for d in (B.SRC, os.path.join(sidelib.HERE, "common"), sidelib.INCLUDE)}
    seen, todo = set(), list(B.sources())
    while todo:
        path = todo.pop()
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
            hits = [p for p in (os.path.join(os.path.dirname(path), name), os.path.join(sidelib.INCLUDE, name)) if os.path.exists(p)]
            assert hits, (path, name)
            hit = os.path.realpath(hits[0])
            if hit not in seen:
                seen.add(hit)
                if os.path.dirname(hit) in followed:
                    todo.append(hit)
    listed = {os.path.realpath(h) for h in B.headers()}
    assert sorted(seen - listed) == []
    assert any(h.endswith("binned_sample.h") for h in seen) and any(h.endswith("isochrones_amd_binned.h") for h in seen)
    # the restated per-sample term says where the other copy is and why it stays there for now
    note = open(os.path.join(sidelib.HERE, "common", "binned_sample.h")).read()
    assert "binned.hip" in note and "pinned" in note
    assert '#include "../common/binned_sample.h"' not in open(libraries.BINNED.sources()[0]).read()
