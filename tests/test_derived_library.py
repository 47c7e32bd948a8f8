"""libiso_derived.so (model-grid columns along a stored chain) builds for gfx950 without a GPU, exports its C ABI and
passes its gates: no AGPRs, no scratch, the register budget of libraries.DERIVED, its waves per SIMD, a clean isa_check scan."""
import ctypes
import os
import re

from isochrones_amd.csrc.libraries import DERIVED as B
from isochrones_amd.csrc import isa_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"iso_derived_version", "iso_derived_last_error", "iso_derived_chain", "iso_derived_chain_host"}


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS
    assert os.path.basename(_built()) == "libiso_derived.so"


def test_every_header_symbol_is_exported():
    path = _built()
    text = open(os.path.join(ROOT, "include", "isochrones_amd_derived.h")).read()
    syms = set(re.findall(r"\b(iso_derived_\w+)\s*\(", text))
    assert syms == SYMBOLS
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    assert lib.iso_derived_chain(None, None, 1, 1, 1, 1, 1, 0, 1, None, 1, None, None, None) == -1      # refused before any device call
    from isochrones_amd import _cabi, _derived_cabi
    assert set(_derived_cabi.EXPORTED_SYMBOLS) == syms
    consts = dict(re.findall(r"#define ISO_DERIVED_(\w+) (\S+)", text))
    assert int(consts["PARAM_MAJOR"]) == _cabi.CHAIN_PARAM_MAJOR and int(consts["ROW_MAJOR"]) == _cabi.CHAIN_ROW_MAJOR
    assert int(consts["MAX_COLS"]) == _derived_cabi.MAX_COLS and int(consts["MAX_COMPS"]) == _derived_cabi.MAX_COMPS
    assert int(consts["ERR_INVALID"].strip("()")) == _derived_cabi.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == _derived_cabi.ERR_HIP
    # the struct of the binding is the header's: four pointers, then n0, n1, nk, Q
    assert [f[0] for f in _derived_cabi.IsoDerivedTable._fields_] == ["cols", "ax0", "ax1", "axk", "n0", "n1", "nk", "Q"]
    assert ctypes.sizeof(_derived_cabi.IsoDerivedTable) == 4 * 8 + 4 * 4


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == {"k_derived_chain"} == set(B.KERNELS)
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["lds"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    path = _built()
    assert isa_check.scan_library(path, jobs=1) == []
