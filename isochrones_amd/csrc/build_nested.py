"""Build libiso_nested.so (nested sampling of a catalog, csrc/nested/) with hipcc for gfx950.

A library of its own, next to libiso_hip.so and libiso_cluster.so: its own object directory (csrc/nested/build/), stamp and
resources JSON.  Its kernels include libiso_hip.so's header-only device code (iso_fast_kernel.h: lnpost_wave and what it
needs), so those headers are part of its source digest.  The same gates as build.py apply: no AGPRs, scratch within the
budget stated below (resources.violations), at most 256 VGPRs and at least two waves per SIMD for every kernel, and a clean
isa_check scan of the generated code."""
from __future__ import annotations

import concurrent.futures
import glob
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "nested")
OUT = os.path.join(HERE, "libiso_nested.so")
OBJDIR = os.path.join(SRC, "build")
STAMP = os.path.join(HERE, "libiso_nested.stamp")
RESOURCES = os.path.join(HERE, "libiso_nested.resources.json")
INCLUDE = os.path.join(HERE, "..", "..", "include")
HEADER = os.path.join(INCLUDE, "isochrones_amd_nested.h")
# (the flags libiso_hip.so's fused kernels are built with: lnpost_wave is the same code here and there)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-Wno-bitwise-instead-of-logical", "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-sched-strategy=max-ilp",
         "-I" + INCLUDE]
#: (parametrisation, stars per system) of every kernel family; each has the instantiations for 1 .. 12 bands
FAMILIES = ((0, 1), (1, 1), (1, 2), (1, 3))
#: every kernel the library compiles (tests/test_nested_catalog_cpu.py pins this set)
KERNELS = tuple("k_catalog_nested<%d, %d, %d>" % (kind, ns, nb) for kind, ns in FAMILIES for nb in range(1, 13))
#: bytes of scratch per lane the family may use, as k_catalog_start has a budget in resources.py: a ratchet, set to what
#: the worst instantiation needs today.  A workgroup here owns a CU's LDS, so one wave per SIMD runs whatever the registers
#: say and the kernel is compiled for 256 VGPRs; at that size only the many-band multiples spill (binary, 12 bands: 8 B;
#: triple, 10 / 11 / 12 bands: 8 / 68 / 148 B), every other instantiation nothing.
SCRATCH_BUDGET = {"k_catalog_nested": 148}
MAX_VGPR = 256
MIN_WAVES = 2


class NestedBuildError(RuntimeError):
    """A kernel of libiso_nested.so outside the budget, or a compile / link failure."""


def sources():
    return sorted(glob.glob(os.path.join(SRC, "*.hip")))


def headers():
    shared = [os.path.join(HERE, "iso_fast_kernel.h"), os.path.join(HERE, "iso_internal.h"), os.path.join(INCLUDE, "isochrones_amd.h")]
    return [HEADER] + sorted(glob.glob(os.path.join(SRC, "*.h"))) + shared + sorted(glob.glob(os.path.join(HERE, "fast", "*.h")))


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
    bad = R.violations(table, scratch_budget=SCRATCH_BUDGET, default_scratch=0, max_agpr=0)
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

    def compile_one(src):
        obj = os.path.join(OBJDIR, os.path.basename(src)[:-4] + ".o")
        p = subprocess.run([cc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj], cwd=SRC,
                           stderr=subprocess.PIPE, text=True, errors="replace")
        return src, obj, p

    jobs = max(1, min(int(os.environ.get("MAX_JOBS", "8")), len(sources())))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        done = list(pool.map(compile_one, sources()))
    for src, obj, p in done:
        rest = [ln for ln in p.stderr.splitlines() if "kernel-resource-usage" not in ln and not R.is_remark_context(ln)]
        if verbose or p.returncode != 0 or any("warning:" in ln or "error:" in ln for ln in rest):
            sys.stderr.write("\n".join(rest) + ("\n" if rest else ""))
        if p.returncode != 0:
            raise NestedBuildError("hipcc failed on %s" % os.path.basename(src))
        with open(obj[:-2] + ".res", "w") as f:
            f.write(p.stderr)
        table.update({k.replace("nestk::", ""): v for k, v in R.parse(p.stderr).items()})
        objs.append(obj)
    for stale in (STAMP, RESOURCES):
        try:
            os.remove(stale)
        except OSError:
            pass
    bad = violations(table)
    if bad:
        raise NestedBuildError("kernel(s) of libiso_nested.so outside the budget:\n  " + "\n  ".join(bad))
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
    from isochrones_amd.csrc import build_nested as B
    print(B.build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
