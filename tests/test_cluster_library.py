"""libiso_cluster.so (the star-cluster likelihood) builds for gfx950 without a GPU, exports its C ABI and passes the same
gates as libiso_hip.so: no AGPRs, no scratch, at most 256 VGPRs, at least two waves per SIMD, a clean isa_check scan."""
import ctypes
import os
import re

from isochrones_amd.csrc.libraries import CLUSTER as B
from isochrones_amd.csrc import isa_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_every_header_symbol_is_exported():
    path = _built()
    text = open(os.path.join(ROOT, "include", "isochrones_amd_cluster.h")).read()
    syms = sorted(set(re.findall(r"\b(iso_cluster_\w+)\s*\(", text)))
    assert set(syms) == {"iso_cluster_version", "iso_cluster_last_error", "iso_cluster_lnlike"}
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)
    from isochrones_amd import _cluster_cabi
    assert set(_cluster_cabi.EXPORTED_SYMBOLS) == set(syms)


def test_resources_and_kernel_set():
    _built()
    table = B.resource_table()
    assert set(table) == {"k_cluster_pairs", "k_cluster_finish"} == set(B.KERNELS)
    for name, r in table.items():
        assert r["agpr"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["waves"] >= 2, (name, r)
    assert B.violations(table) == []


def test_generated_code_is_clean():
    path = _built()
    assert isa_check.scan_library(path, jobs=1) == []
