"""libiso_population.so (a batch of coeval single or binary systems on the model and the BC grid) builds for gfx950 without
a GPU, exports its C ABI and passes its gates: no AGPRs, no scratch, the register budget of libraries.POPULATION, its waves
per SIMD, a clean isa_check scan.  The library joins the build through libraries.BUILD_ORDER; libraries.ALL stays the six."""
import ctypes
import itertools
import os
import re
import subprocess

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import isa_check, libraries
from isochrones_amd.csrc.libraries import POPULATION as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert os.path.basename(_built()) == "libiso_population.so"
    src = open(os.path.join(B.SRC, "population.hip")).read()
    assert not re.search(r"\bfma\s*\(", src)                    # the header's arithmetic has no fused multiply-add


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _population_cabi as pc
    text = open(os.path.join(ROOT, "include", "isochrones_amd_population.h")).read()
    syms = set(re.findall(r"\b(iso_population_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(pc.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(pc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_POPULATION_(\w+) (\S+)", text))
    assert int(consts["MAX_COLS"]) == pc.MAX_COLS == 32 and int(consts["MAX_BANDS"]) == pc.MAX_BANDS == 32
    assert int(consts["MAX_COMPS"]) == pc.MAX_COMPS == 2
    assert int(consts["MAX_BLOCKS"]) == pc.MAX_BLOCKS == 2048
    assert "constexpr int MAX_BLOCKS = ISO_POPULATION_MAX_BLOCKS;" in open(os.path.join(B.SRC, "population.hip")).read()
    assert int(consts["ERR_INVALID"].strip("()")) == pc.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == pc.ERR_HIP
    assert ctypes.sizeof(pc.IsoPopulationModelTable) == 4 * 8 + 8 * 4
    assert ctypes.sizeof(pc.IsoPopulationBcTable) == 5 * 8 + 6 * 4
    assert ctypes.sizeof(pc.IsoPopulationOut) == 5 * 8
    assert os.path.samefile(path, pc.library_path())
    assert pc.EXPORTED_SYMBOLS[:2] == ("iso_population_version", "iso_population_last_error")
    assert lib.iso_population_version


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_population_eval"}
    assert B.MIN_WAVES >= 2
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []


def test_build_order_is_all_and_the_new_library():
    assert [s.name for s in libraries.ALL] == ["cluster", "nested", "solve", "diag", "derived", "predict"]
    assert libraries.BUILD_ORDER == libraries.ALL + (B,) and B.name == "population"
    for a, b in itertools.combinations((main,) + libraries.BUILD_ORDER, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    assert len({s.source_digest() for s in libraries.BUILD_ORDER}) == len(libraries.BUILD_ORDER)
    assert not any("population" in os.path.basename(s) for s in main.sources())
    assert os.path.exists(B.HEADER) and B.HEADER in B.headers()
    assert [os.path.basename(h) for h in B.headers()] == ["isochrones_amd_population.h", "grid_cell.h", "grid_interp.h", "last_error.h"]
    # what build() and the command line iterate
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libraries.BUILD_ORDER" in entry and "libraries.ALL" not in entry
