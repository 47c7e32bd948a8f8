"""libiso_binfit.so (the moments of the stars' posterior cell probabilities under a binned population) builds for gfx950
without a GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.BINFIT, its
waves per SIMD, a clean isa_check scan.  The library joins the build through libraries.LATEST; the earlier tuples stay what
they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries, sidelib
from isochrones_amd.csrc.libraries import BINFIT as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.BINNED.FLAGS == libraries.SHRINK.FLAGS
    assert os.path.basename(_built()) == "libiso_binfit.so"
    assert [os.path.basename(s) for s in B.sources()] == ["binfit.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path
    src = open(B.sources()[0]).read()
    assert '#include "isochrones_amd_binfit.h"' in src and '#include "../common/last_error.h"' in src
    assert "ISO_BINNED_MAX_CELLS" in src
    header = open(B.HEADER).read()
    assert '#include "isochrones_amd_binned.h"' in header and "Summation order" in header


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _binfit_cabi as fc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_binfit.h")).read()
    body = text.split("#ifndef")[1]
    syms = set(re.findall(r"\b(iso_binfit_\w+)\s*\(", body))
    assert syms == set(fc.EXPORTED_SYMBOLS) and len(syms) == 5
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(fc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_BINFIT_(\w+) (\S+)", body))
    assert int(consts["CHUNK"]) == fc.CHUNK == 4096 and int(consts["TILE"]) == fc.TILE and fc.CHUNK % fc.TILE == 0
    assert int(consts["ERR_INVALID"].strip("()")) == fc.ERR_INVALID and int(consts["ERR_HIP"].strip("()")) == fc.ERR_HIP
    from isochrones_amd import _binned_cabi as bc
    assert fc.MAX_CELLS == bc.MAX_CELLS == 64
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1))
    assert args("iso_binfit_moments") == args("iso_binfit_moments_host")
    assert os.path.samefile(path, fc.library_path())
    assert fc.EXPORTED_SYMBOLS[:2] == ("iso_binfit_version", "iso_binfit_last_error")
    lib.iso_binfit_version.restype = ctypes.c_char_p
    assert lib.iso_binfit_version()
    # the workspace: [H][chunks][B + B (B + 1) / 2] doubles and the chunks' live counts, two int32 a double
    ws = lib.iso_binfit_workspace_doubles
    ws.restype, ws.argtypes = ctypes.c_int64, [ctypes.c_int32] * 3 + [ctypes.c_int]
    assert ws(64, 4097, 3, 1) == 3 * 2 * (64 + 2080) + 3 and ws(64, 4096, 3, 0) == 3 * 64 + 2 and ws(1, 1, 1, 1) == 3
    assert ws(65, 10, 1, 1) == 0 and ws(0, 10, 1, 1) == 0 and ws(8, 0, 1, 1) == 0 and ws(8, 10, 0, 1) == 0


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_binfit_partial", "k_binfit_total"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    # max_vgpr is the occupancy step the partial kernel compiles to: 512 registers a SIMD lane, in granules of 8.  Its waves
    # are set by the LDS (a tile of 64 stars x 65 doubles, the row's heights, the tile's s1), below the 64 KB a launch gets
    # without asking
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_binfit_partial"]["waves"] == B.MIN_WAVES == 4
    assert 64 * 65 * 8 <= table["k_binfit_partial"]["lds"] <= 64 * 65 * 8 + 1024 < 65536
    assert table["k_binfit_total"]["waves"] == 8 and table["k_binfit_total"]["lds"] == 0
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.LATEST and B.name == "binfit"
    assert B not in libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert [s.name for s in libraries.LATEST[:3]] == ["shrink", "draw", "binfit"] and len(EVERY) >= 15
    assert len({s.name for s in EVERY}) == len(EVERY)
    for a, b in itertools.combinations((main,) + EVERY, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in EVERY}) == len(EVERY)
    assert not any("binfit" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_binfit.h", "isochrones_amd_binned.h",
                                                          "isochrones_amd_hier.h", "last_error.h"]
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST" in entry
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "isochrones_amd/csrc/libiso_binfit.resources.json" in ignored and "*.stamp" in ignored
    import isochrones_amd as ia
    from isochrones_amd import binfit
    assert ia.BinnedFit is binfit.BinnedFit


def test_the_digest_covers_every_header_the_sources_reach():
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
    assert any(h.endswith("isochrones_amd_binned.h") for h in seen) and any(h.endswith("isochrones_amd_hier.h") for h in seen)
