"""Build libiso_predict.so (posterior-predictive check of a stored chain, csrc/predict/) with hipcc for gfx950.

A library of its own, next to libiso_hip.so: its own object directory (csrc/predict/build/), stamp and resources JSON.  The
same gates as build.py apply, imported from there: no AGPRs and a scratch budget of 0 bytes (resources.violations), at most
MAX_VGPR VGPRs and at least MIN_WAVES waves per SIMD for every kernel, and a clean isa_check scan of the generated code."""
from __future__ import annotations

import glob
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "predict")
OUT = os.path.join(HERE, "libiso_predict.so")
OBJDIR = os.path.join(SRC, "build")
STAMP = os.path.join(HERE, "libiso_predict.stamp")
RESOURCES = os.path.join(HERE, "libiso_predict.resources.json")
INCLUDE = os.path.join(HERE, "..", "..", "include")
HEADER = os.path.join(INCLUDE, "isochrones_amd_predict.h")
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a sample's values are bit-identical in any batch, ensemble range and layout)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function", "-I" + INCLUDE]
#: every kernel the library compiles (tests/test_predict_library.py pins this set)
KERNELS = ("k_predict_chain",)
#: k_predict_chain compiles to 239 VGPRs, no scratch and 2 waves per SIMD.  A sample holds the brackets and weights of a 4-D
#: cell, eight band accumulators, four corners of eight bands in flight and the model cell's 32 values; the call's 60-odd
#: uniform values (two tables, strides, outputs) are staged in LDS because as kernel arguments they overflow the SGPR file and
#: their spill slots count as scratch.  The workgroup is two waves, so the budget is the 2-waves-per-SIMD one: 256 VGPRs
MAX_VGPR = 256
MIN_WAVES = 2
SCRATCH_BUDGET = 0


class PredictBuildError(RuntimeError):
    """A kernel of libiso_predict.so outside the budget, or a compile / link failure."""


def sources():
    return sorted(glob.glob(os.path.join(SRC, "*.hip")))


def headers():
    return [HEADER] + sorted(glob.glob(os.path.join(SRC, "*.h")))


def source_digest() -> str:
    from .build import compiler_version
    h = hashlib.sha256((repr(FLAGS) + compiler_version()).encode())
    for path in sources() + headers() + [os.path.abspath(__file__), os.path.join(HERE, "resources.py"),
                                         os.path.join(HERE, "isa_check.py")]:
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def up_to_date() -> bool:
    from .build import file_sha256
    try:
        src, so = open(STAMP).read().split()[:2]
    except (OSError, ValueError):
        return False
    return os.path.exists(OUT) and os.path.exists(RESOURCES) and src == source_digest() and so == file_sha256(OUT)


def resource_table() -> dict:
    with open(RESOURCES) as f:
        return json.load(f)


def violations(table: dict) -> list:
    from . import resources as R
    bad = R.violations(table, scratch_budget={}, default_scratch=SCRATCH_BUDGET, max_agpr=0)
    for name, r in sorted(table.items()):
        if r.get("vgpr", 0) > MAX_VGPR:
            bad.append("%s: %d VGPRs (limit %d)" % (name, r["vgpr"], MAX_VGPR))
        if r.get("waves", 0) < MIN_WAVES:
            bad.append("%s: %d waves per SIMD (at least %d)" % (name, r.get("waves", 0), MIN_WAVES))
    return bad


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile, gate and link when the sources changed; return the library path."""
    from . import resources as R
    from . import isa_check as I
    from .build import hipcc, file_sha256
    digest = source_digest()
    if not force and up_to_date():
        return OUT
    os.makedirs(OBJDIR, exist_ok=True)
    cc = hipcc()
    objs, table = [], {}
    for src in sources():
        obj = os.path.join(OBJDIR, os.path.basename(src)[:-4] + ".o")
        p = subprocess.run([cc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj], cwd=SRC,
                           stderr=subprocess.PIPE, text=True, errors="replace")
        rest = [ln for ln in p.stderr.splitlines() if "kernel-resource-usage" not in ln and not R.is_remark_context(ln)]
        if verbose or p.returncode != 0 or any("warning:" in ln or "error:" in ln for ln in rest):
            sys.stderr.write("\n".join(rest) + ("\n" if rest else ""))
        if p.returncode != 0:
            raise PredictBuildError("hipcc failed on %s" % os.path.basename(src))
        with open(obj[:-2] + ".res", "w") as f:
            f.write(p.stderr)
        table.update(R.parse(p.stderr))
        objs.append(obj)
    for stale in (STAMP, RESOURCES):
        try:
            os.remove(stale)
        except OSError:
            pass
    bad = violations(table)
    if bad:
        raise PredictBuildError("kernel(s) of libiso_predict.so outside the budget:\n  " + "\n  ".join(bad))
    faults = [tuple(x) for obj in objs for x in I.scan_library(obj, jobs=1)]
    if faults:
        raise I.IsaFault(I.render(faults))
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs, cwd=SRC)
    with open(RESOURCES, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
    with open(STAMP, "w") as f:
        f.write(digest + "\n" + file_sha256(OUT) + "\n")
    return OUT


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from isochrones_amd.csrc import build_predict as B
    print(B.build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
