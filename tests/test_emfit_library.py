"""libiso_emfit.so (a batch of weighted EM fits of a binned population's cell masses, and bootstrap weights) builds for
gfx950 without a GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, no spill, the register budget of
libraries.EMFIT, its waves per SIMD, a clean isa_check scan.  The library joins the build through libraries.LATEST as its
fourth member; the earlier tuples stay what they were."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries, sidelib
from isochrones_amd.csrc.libraries import EMFIT as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST
RUN = tuple("k_emfit_run<%d>" % p for p in (8, 16, 32, 64))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert B.FLAGS == libraries.BINNED.FLAGS == libraries.SHRINK.FLAGS == libraries.BINFIT.FLAGS
    assert os.path.basename(_built()) == "libiso_emfit.so"
    assert [os.path.basename(s) for s in B.sources()] == ["emfit.hip"]
    for path in B.sources() + [h for h in B.headers() if os.path.basename(os.path.dirname(h)) == "common"]:
        src = open(path).read()
        assert not re.search(r"\bfma\s*\(", src), path               # the header's arithmetic has no fused multiply-add
        assert not re.search(r"atomic", src), path
    src = open(B.sources()[0]).read()
    assert '#include "isochrones_amd_emfit.h"' in src and '#include "../common/last_error.h"' in src
    assert '#include "../common/philox.h"' in src and '#include "../common/wave_reduce.h"' in src
    assert "ISO_BINNED_MAX_CELLS" in src and "wave_sum(" in src and "__restrict__" not in src.split("k_emfit_weights")[0]
    header = open(B.HEADER).read()
    assert '#include "isochrones_amd_binned.h"' in header and "Summation order" in header and "Definition." in header


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _emfit_cabi as ec
    text = open(os.path.join(ROOT, "include", "isochrones_amd_emfit.h")).read()
    body = text.split("#ifndef")[1]
    syms = set(re.findall(r"\b(iso_emfit_\w+)\s*\(", body))
    assert syms == set(ec.EXPORTED_SYMBOLS) and len(syms) == 6
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(ec.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_EMFIT_(\w+) (\S+)", body))
    assert int(consts["ERR_INVALID"].strip("()")) == ec.ERR_INVALID and int(consts["ERR_HIP"].strip("()")) == ec.ERR_HIP
    assert [int(consts[k]) for k in ("RUNNING", "CONVERGED", "MAX_ITER", "EMPTY")] == [ec.RUNNING, ec.CONVERGED, ec.MAX_ITER,
                                                                                      ec.EMPTY] == [0, 1, 2, 3]
    assert [int(consts[k]) for k in ("POISSON", "EXP")] == [ec.POISSON, ec.EXP]
    assert int(consts["LANES"]) == ec.LANES == 256 and int(consts["LAUNCH_WORK"]) == ec.LAUNCH_WORK == 2 ** 31
    assert int(consts["PHILOX_TAG"], 16) == ec.PHILOX_TAG == 0xB7 and int(consts["POISSON_TERMS"]) == ec.POISSON_TERMS == 18
    from isochrones_amd import _binned_cabi as bc
    assert ec.MAX_CELLS == bc.MAX_CELLS == 64
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1))
    assert args("iso_emfit_run") == args("iso_emfit_run_host")
    assert args("iso_emfit_weights") == args("iso_emfit_weights_host")
    assert os.path.samefile(path, ec.library_path())
    assert ec.EXPORTED_SYMBOLS[:2] == ("iso_emfit_version", "iso_emfit_last_error")
    lib.iso_emfit_version.restype = ctypes.c_char_p
    assert lib.iso_emfit_version()


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == set(RUN) | {"k_emfit_weights"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    # max_vgpr is the occupancy step the widest instantiation compiles to: 512 registers a SIMD lane, in granules of 8.  A
    # lane's sums alone are two registers a cell of the padded grid
    assert B.MAX_VGPR == 512 // B.MIN_WAVES // 8 * 8 and table["k_emfit_run<64>"]["waves"] == B.MIN_WAVES == 2
    for pad, name in zip((8, 16, 32, 64), RUN):
        assert table[name]["vgpr"] >= 2 * pad and 0 < table[name]["lds"] <= 4096, (name, table[name])
    assert [table[n]["waves"] for n in RUN] == sorted((table[n]["waves"] for n in RUN), reverse=True)
    assert table["k_emfit_run<32>"]["waves"] >= 3
    assert table["k_emfit_weights"]["waves"] == 8 and table["k_emfit_weights"]["lds"] == 0
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_lists():
    assert B in libraries.LATEST and B.name == "emfit" and libraries.LATEST[3].name == "emfit"
    assert B not in libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER
    assert [s.name for s in libraries.LATEST[:4]] == ["shrink", "draw", "binfit", "emfit"] and len(EVERY) >= 16
    assert len({s.name for s in EVERY}) == len(EVERY)
    for a, b in itertools.combinations((main,) + EVERY, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in EVERY}) == len(EVERY)
    assert not any("emfit" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_emfit.h", "isochrones_amd_binned.h",
                                                          "isochrones_amd_hier.h", "last_error.h", "philox.h",
                                                          "wave_reduce.h"]
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER + libraries.LATEST" in entry
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "isochrones_amd/csrc/libiso_emfit.resources.json" in ignored and "*.stamp" in ignored
    import isochrones_amd as ia
    from isochrones_amd import emfit
    assert ia.BinnedBootstrap is emfit.BinnedBootstrap


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
    assert any(h.endswith("isochrones_amd_binned.h") for h in seen) and any(h.endswith("philox.h") for h in seen)
