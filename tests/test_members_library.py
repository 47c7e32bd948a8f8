"""libiso_members.so (per-star moments of the star-cluster likelihood's integrand) builds for gfx950 without a GPU, exports its C
ABI and passes its gates: no AGPRs, no scratch, no spilled VGPR, the register budget of libraries.MEMBERS, its waves per SIMD, a
clean isa_check scan.  The library joins the build through libraries.LATEST as its fifth member; the earlier tuples stay what
they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries, sidelib
from isochrones_amd.csrc.libraries import MEMBERS as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.CLUSTER.FLAGS                           # the cell arithmetic is built as the likelihood's is
    assert os.path.basename(_built()) == "libiso_members.so"
    assert [os.path.basename(s) for s in B.sources()] == ["members.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path
    src = open(B.sources()[0]).read()
    assert '#include "isochrones_amd_members.h"' in src and '#include "../common/last_error.h"' in src
    assert "hipMalloc" not in src and "Synchronize" not in src           # allocates nothing, does not synchronise
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src           # 32 bands: more than 64 KB of LDS
    header = open(B.HEADER).read()
    assert "Summation order" in header and "Definition." in header and "e == 0" in header


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _members_cabi as mc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_members.h")).read()
    body = text.split("#ifndef")[1]
    syms = set(re.findall(r"\b(iso_members_\w+)\s*\(", body))
    assert syms == set(mc.EXPORTED_SYMBOLS) and len(syms) == 4
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(mc.EXPORTED_SYMBOLS)
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1))
    assert args("iso_members_moments") == args("iso_members_moments_host")
    cluster = open(os.path.join(ROOT, "include", "isochrones_amd_cluster.h")).read()
    inputs = re.sub(r"\s+", " ", re.search(r"\bint iso_cluster_lnlike\((.*?)double\* work", cluster, re.S).group(1))
    assert args("iso_members_moments").startswith(inputs)                # exactly the likelihood's inputs
    assert os.path.samefile(path, mc.library_path())
    assert mc.EXPORTED_SYMBOLS[:2] == ("iso_members_version", "iso_members_last_error")
    lib.iso_members_version.restype = ctypes.c_char_p
    assert lib.iso_members_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_members_pairs", "k_members_finish"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
    # max_vgpr is the occupancy step the pairs kernel compiles to: 512 registers a SIMD lane, in granules of 8
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8
    # six running trapezoids and six previous products a lane, two registers each
    assert table["k_members_pairs"]["vgpr"] >= 24
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.LATEST and B.name == "members" and libraries.LATEST[4].name == "members"
    assert B not in libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert [s.name for s in libraries.LATEST[:4]] == ["shrink", "draw", "binfit", "emfit"] and len(EVERY) >= 17
    assert [s.name for s in libraries.ALL] == ["cluster", "nested", "solve", "diag", "derived", "predict"]
    assert [s.name for s in libraries.BUILD_ORDER[6:]] == ["population"] and [s.name for s in libraries.ADDED] == ["hier"]
    assert [s.name for s in libraries.NEWER] == ["select", "reweight", "relation", "binned"]
    assert len({s.name for s in EVERY}) == len(EVERY)
    for a, b in itertools.combinations((main,) + EVERY, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in EVERY}) == len(EVERY)
    assert not any("members" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_members.h", "last_error.h"]
    assert libraries.CLUSTER.kernels == ("k_cluster_finish", "k_cluster_pairs")      # the likelihood's library is untouched
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST" in entry
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "isochrones_amd/csrc/libiso_members.resources.json" in ignored and "*.stamp" in ignored
    import isochrones_amd as ia
    from isochrones_amd import cluster
    assert ia.combine_star_moments is cluster.combine_star_moments


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
