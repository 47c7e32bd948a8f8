"""libiso_binned.so (the population likelihood for a density that is piecewise constant on a grid of bins) builds for
gfx950 without a GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of
libraries.BINNED, its waves per SIMD, a clean isa_check scan.  The library joins the build through libraries.NEWER; hier,
select, reweight and relation stay what they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries
from isochrones_amd.csrc.libraries import BINNED as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.HIER.FLAGS == libraries.SELECT.FLAGS == libraries.REWEIGHT.FLAGS == libraries.RELATION.FLAGS
    assert os.path.basename(_built()) == "libiso_binned.so"
    assert [os.path.basename(s) for s in B.sources()] == ["binned.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path                  # every sum in a fixed order
    src = open(B.sources()[0]).read()
    # the kinds 1 .. 8 are the shared arithmetic; the chain's strides and the last error are the shared headers'
    assert '#include "../common/family_lnf.h"' in src and '#include "../common/chain_view.h"' in src
    assert "feh_shape" not in src and "thread_local" not in src


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _binned_cabi as bc, _hier_cabi as hc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_binned.h")).read()
    assert '#include "isochrones_amd_hier.h"' in text
    syms = set(re.findall(r"\b(iso_binned_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(bc.EXPORTED_SYMBOLS) and len(syms) == 6
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(bc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_BINNED_(\w+) (\S+)", text))
    assert int(consts["MAX_CELLS"]) == bc.MAX_CELLS == 64 and int(consts["MAX_AXES"]) == bc.MAX_AXES == 2
    assert int(consts["ROW_TILE"]) == bc.ROW_TILE == 8
    assert int(consts["ERR_INVALID"].strip("()")) == bc.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == bc.ERR_HIP
    # the records and the column descriptors are the hierarchical library's, as they are: the header defines no type
    assert bc.RECORD is hc.RECORD and bc.IsoHierColumn is hc.IsoHierColumn and bc.MAX_COLS == hc.MAX_COLS == 4
    assert not re.search(r"typedef struct", text.split("#ifndef")[1])
    # a device entry and its host entry take the same arguments
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1))
    assert args("iso_binned_compress") == args("iso_binned_compress_host")
    assert args("iso_binned_lnlike") == args("iso_binned_lnlike_host")
    assert os.path.samefile(path, bc.library_path())
    assert bc.EXPORTED_SYMBOLS[:2] == ("iso_binned_version", "iso_binned_last_error")
    lib.iso_binned_version.restype = ctypes.c_char_p
    assert lib.iso_binned_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_binned_compress", "k_binned_rows", "k_binned_total"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
        # nothing spills to memory.  The compression kernel's argument block overflows the SGPR file into VGPR lanes, as
        # k_relation_stars's (43) and k_reweight_weights's (49) do: pinned, so that growth is noticed
        assert r["sgpr_spill"] <= (24 if name == "k_binned_compress" else 0), (name, r)
    # max_vgpr is the occupancy step the compression kernel compiles to: 512 registers a SIMD lane, in granules of 8
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_binned_compress"]["waves"] == B.MIN_WAVES
    # the contraction is the call that repeats: it keeps the full occupancy
    assert table["k_binned_rows"]["waves"] == 8 and table["k_binned_total"]["waves"] == 8
    # LDS: a tile's 256 (weight, cell) pairs, the edges and the records; the row tile's u and u * u; the reduction
    assert table["k_binned_compress"]["lds"] <= 5120 and table["k_binned_rows"]["lds"] <= 8448
    assert table["k_binned_total"]["lds"] <= 64
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.NEWER and B.name == "binned"
    for earlier in (libraries.SELECT, libraries.REWEIGHT, libraries.RELATION):
        assert earlier in libraries.NEWER
    every = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert len({s.name for s in every}) == len(every)
    for a, b in itertools.combinations((main,) + every, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in every}) == len(every)
    assert not any("binned" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_binned.h", "isochrones_amd_hier.h", "family_lnf.h",
                                                          "grid_cell.h", "last_error.h", "wave_reduce.h", "hier_columns.h",
                                                          "chain_view.h", "hier_block.h"]
    # what build() and the command line iterate, and what git ignores
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER" in entry
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "isochrones_amd/csrc/libiso_binned.resources.json" in ignored and "*.stamp" in ignored
