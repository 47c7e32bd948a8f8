"""libiso_predict.so (posterior-predictive check of a stored chain) builds for gfx950 without a GPU, exports its C ABI and
passes its gates: no AGPRs, no scratch, the register budget of libraries.PREDICT, its waves per SIMD, a clean isa_check scan."""
import ctypes
import os
import re

from isochrones_amd.csrc.libraries import PREDICT as B
from isochrones_amd.csrc import isa_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_builds_for_gfx950():
    assert "--offload-arch=gfx950" in B.FLAGS and "-ffp-contract=off" in B.FLAGS and "-fno-fast-math" in B.FLAGS
    assert os.path.basename(_built()) == "libiso_predict.so"


def test_exports_exactly_the_bound_symbols():
    path = _built()
    from isochrones_amd import _cabi, _predict_cabi
    text = open(os.path.join(ROOT, "include", "isochrones_amd_predict.h")).read()
    syms = set(re.findall(r"\b(iso_predict_\w+)\s*\(", text.split("#ifndef")[1]))
    assert syms == set(_predict_cabi.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and "iso_" in ln.split()[-1]}
    assert exported == set(_predict_cabi.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_PREDICT_(\w+) (\S+)", text))
    assert int(consts["PARAM_MAJOR"]) == _cabi.CHAIN_PARAM_MAJOR and int(consts["ROW_MAJOR"]) == _cabi.CHAIN_ROW_MAJOR
    assert int(consts["MAX_BANDS"]) == _predict_cabi.MAX_BANDS == 32 and int(consts["MAX_COMPS"]) == _predict_cabi.MAX_COMPS
    assert int(consts["LANES"]) == _predict_cabi.LANES and int(consts["NSPEC"]) == _predict_cabi.NSPEC
    assert int(consts["MAX_BLOCKS"]) == _predict_cabi.MAX_BLOCKS == 2048
    assert "constexpr int MAX_BLOCKS = ISO_PREDICT_MAX_BLOCKS;" in open(os.path.join(B.SRC, "predict.hip")).read()
    assert int(consts["ERR_INVALID"].strip("()")) == _predict_cabi.ERR_INVALID
    assert int(consts["ERR_HIP"].strip("()")) == _predict_cabi.ERR_HIP
    assert ctypes.sizeof(_predict_cabi.IsoPredictModelTable) == 4 * 8 + 4 * 4
    assert ctypes.sizeof(_predict_cabi.IsoPredictBcTable) == 5 * 8 + 6 * 4
    assert ctypes.sizeof(_predict_cabi.IsoPredictOut) == 7 * 8
    assert os.path.samefile(path, _predict_cabi.library_path())


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == set(B.KERNELS) == {"k_predict_chain"}
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == B.SCRATCH_BUDGET == 0, (name, r)
        assert r["vgpr"] <= B.MAX_VGPR and r["waves"] >= B.MIN_WAVES, (name, r)
        assert r["vgpr_spill"] == 0, (name, r)
    assert B.violations(table) == []
    bad = {"k": dict(agpr=0, scratch=16, vgpr=300, waves=1, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0)}
    assert len(B.violations(bad)) >= 3


def test_generated_code_is_clean():
    assert isa_check.scan_library(_built(), jobs=1) == []
