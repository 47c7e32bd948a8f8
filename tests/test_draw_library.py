"""libiso_draw.so (the random draws of synthetic populations and injection sets) builds for gfx950 without a GPU, exports
its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.DRAW, its waves per SIMD, a clean
isa_check scan.  The library joins the build through libraries.LATEST; the earlier tuples stay what they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries, sidelib
from isochrones_amd.csrc.libraries import DRAW as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.HIER.FLAGS == libraries.SHRINK.FLAGS
    assert os.path.basename(_built()) == "libiso_draw.so"
    assert [os.path.basename(s) for s in B.sources()] == ["draw.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path
    src = open(B.sources()[0]).read()
    for shared in ("last_error.h", "ndtri.h", "philox.h"):
        assert '#include "../common/%s"' % shared in src
    # the device's own inverse is not used, and there is no rejection loop
    assert "normcdfinv" not in src and "while" not in src
    ndtri = open(os.path.join(sidelib.HERE, "common", "ndtri.h")).read()
    assert "AS 241" in ndtri and "PPND16" in ndtri and "__host__ __device__" in ndtri and "normcdfinv(" not in ndtri
    philox = open(os.path.join(sidelib.HERE, "common", "philox.h")).read()
    assert "__host__ __device__" in philox and "0xD2511F53u" in philox and "0xCD9E8D57u" in philox


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _draw_cabi as dc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_draw.h")).read()
    body = text.split("#ifndef")[1]
    syms = set(re.findall(r"\b(iso_draw_\w+)\s*\(", body))
    assert syms == set(dc.EXPORTED_SYMBOLS) and len(syms) == 5
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(dc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_DRAW_(\w+) (\S+)", body))
    assert int(consts["MAX_COLS"]) == dc.MAX_COLS == 8 and int(consts["MAX_BINS"]) == dc.MAX_BINS == 64
    assert int(consts["NPAR"]) == dc.NPAR and int(consts["PHILOX_TAG"], 16) == dc.PHILOX_TAG
    assert int(consts["MAX_BLOCKS"]) == dc.MAX_BLOCKS == 4096
    assert "constexpr int MAX_BLOCKS = ISO_DRAW_MAX_BLOCKS;" in open(B.sources()[0]).read()
    assert dc.PHILOX_TAG not in (0x51, 0x4E)                        # the samplers' and the nested sampler's
    assert int(consts["ERR_INVALID"].strip("()")) == dc.ERR_INVALID and int(consts["ERR_HIP"].strip("()")) == dc.ERR_HIP
    kinds = ("FLAT", "FLATLOG", "POWERLAW", "GAUSS", "LOGNORMAL", "CHABRIER", "FEH", "TRUNCGAUSS", "LINGAUSS", "TABLE", "CONSTANT")
    assert [int(consts[k]) for k in kinds] == [getattr(dc, k) for k in kinds] == list(range(1, 12))
    from isochrones_amd import _hier_cabi as hc, _relation_cabi as rc
    assert (dc.FLAT, dc.TRUNCGAUSS, dc.LINGAUSS) == (hc.FLAT, hc.TRUNCGAUSS, rc.LINGAUSS)
    assert dc.RECORD.itemsize == 112 and dc.RECORD.fields["lo"][1] == 16 and dc.RECORD.fields["p"][1] == 32
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1))
    assert args("iso_draw_systems") == args("iso_draw_systems_host")
    assert os.path.samefile(path, dc.library_path())
    assert dc.EXPORTED_SYMBOLS[:2] == ("iso_draw_version", "iso_draw_last_error")
    lib.iso_draw_version.restype = ctypes.c_char_p
    assert lib.iso_draw_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_draw_systems"}
    assert B.MIN_WAVES >= 2
    r = table["k_draw_systems"]
    assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, r
    assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, r
    assert r["vgpr_spill"] == 0, r
    # the system's values stay in registers: no LDS.  A record of the argument block overflows the SGPR file into VGPR
    # lanes, not into memory: pinned, so that growth is noticed
    assert r["lds"] == 0 and r["sgpr_spill"] <= 17, r
    # max_vgpr is the occupancy step the kernel compiles to: 512 registers a SIMD lane, in granules of 8
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and r["waves"] == B.MIN_WAVES == 4
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.LATEST and B.name == "draw"
    assert B not in libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert [s.name for s in libraries.LATEST[:2]] == ["shrink", "draw"] and len(EVERY) >= 14
    assert len({s.name for s in EVERY}) == len(EVERY)
    for a, b in itertools.combinations((main,) + EVERY, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in EVERY}) == len(EVERY)
    assert not any("draw" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_draw.h", "last_error.h", "ndtri.h", "philox.h"]
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST" in entry
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "isochrones_amd/csrc/libiso_draw.resources.json" in ignored and "*.stamp" in ignored
    # the samplers' own copy of the rounds stays where it is: its digest feeds the fused kernels
    assert "philox.h" not in open(os.path.join(sidelib.HERE, "fast", "sampler.h")).read()


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
    assert any(h.endswith("ndtri.h") for h in seen) and any(h.endswith("philox.h") for h in seen)
