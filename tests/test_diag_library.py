"""libiso_diag.so (per-star chain convergence diagnostics) builds for gfx950 without a GPU, exports its C ABI and passes
its gates: no AGPRs, no scratch, the register budget of libraries.DIAG, eight waves per SIMD, a clean isa_check scan."""
import ctypes
import os
import re

from isochrones_amd.csrc.libraries import DIAG as B
from isochrones_amd.csrc import isa_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"iso_diag_version", "iso_diag_last_error", "iso_diag_chain", "iso_diag_chain_host"}


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS
    assert os.path.basename(_built()) == "libiso_diag.so"


def test_every_header_symbol_is_exported():
    path = _built()
    text = open(os.path.join(ROOT, "include", "isochrones_amd_diag.h")).read()
    syms = set(re.findall(r"\b(iso_diag_\w+)\s*\(", text))
    assert syms == SYMBOLS
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    from isochrones_amd import _cabi, _diag_cabi
    assert set(_diag_cabi.EXPORTED_SYMBOLS) == syms
    consts = dict(re.findall(r"#define ISO_DIAG_(\w+) (\S+)", text))
    assert int(consts["PARAM_MAJOR"]) == _cabi.CHAIN_PARAM_MAJOR and int(consts["ROW_MAJOR"]) == _cabi.CHAIN_ROW_MAJOR
    assert int(consts["NOUT"]) == _diag_cabi.NOUT
    assert [int(consts[k]) for k in ("TAU", "WINDOW", "WINDOW_OK", "ESS", "RHAT")] == [
        _diag_cabi.TAU, _diag_cabi.WINDOW, _diag_cabi.WINDOW_OK, _diag_cabi.ESS, _diag_cabi.RHAT]
    assert float(consts["DEFAULT_C"]) == _diag_cabi.DEFAULT_C and int(consts["DEFAULT_MAX_LAG"]) == _diag_cabi.DEFAULT_MAX_LAG


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == {"k_diag_chain"} == set(B.KERNELS)
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["lds"] == 0, (name, r)          # no static LDS in front of the dynamic region (its base stays aligned)
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    path = _built()
    assert isa_check.scan_library(path, jobs=1) == []
