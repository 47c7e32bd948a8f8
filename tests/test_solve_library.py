"""libiso_solve.so (the exact (mass, age, [Fe/H]) -> EEP solve) builds for gfx950 without a GPU, exports its C ABI and
passes its gates: no AGPRs, no scratch, the register budget of libraries.SOLVE, at least two waves per SIMD, a clean isa_check
scan, and no scalar-memory write in its sources."""
import ctypes
import glob
import os
import re

from isochrones_amd.csrc.libraries import SOLVE as B
from isochrones_amd.csrc import isa_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"iso_solve_version", "iso_solve_last_error", "iso_solve_last_axis", "iso_solve_last_axis_host"}


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS
    assert os.path.basename(_built()) == "libiso_solve.so"


def test_every_header_symbol_is_exported():
    path = _built()
    text = open(os.path.join(ROOT, "include", "isochrones_amd_solve.h")).read()
    syms = set(re.findall(r"\b(iso_solve_\w+)\s*\(", text))
    assert syms == SYMBOLS
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    from isochrones_amd import _solve_cabi
    assert set(_solve_cabi.EXPORTED_SYMBOLS) == syms
    assert _solve_cabi.HOLE_BIT == int(re.search(r"#define ISO_SOLVE_HOLE_BIT (0x[0-9a-fA-F]+)", text).group(1), 16)


def test_table_struct_matches_the_header():
    from isochrones_amd import _solve_cabi
    t = _solve_cabi.IsoSolveTable
    assert [f[0] for f in t._fields_] == ["col", "ax0", "ax1", "axk", "range", "n0", "n1", "nk"]
    assert ctypes.sizeof(t) == 5 * 8 + 3 * 4 + 4          # five pointers, three int32, padded to 8


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == {"k_solve_last_axis"} == set(B.KERNELS)
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    path = _built()
    assert isa_check.scan_library(path, jobs=1) == []


def test_sources_hold_no_scalar_memory_write():
    words = ["s_" + w for w in ("store_", "buffer_store_", "scratch_store_", "atomic_", "buffer_atomic_", "dcache_wb",
                                "dcache_discard")]
    files = glob.glob(os.path.join(B.SRC, "*.hip")) + glob.glob(os.path.join(B.SRC, "*.h")) + [B.HEADER]
    assert files
    for f in files:
        text = open(f).read().lower()
        assert not any(w in text for w in words), f
