"""The one builder of the side libraries (libiso_cluster.so, libiso_nested.so, ...: the specs are in libraries.py).

Each is a library of its own next to libiso_hip.so: sources in csrc/<name>/, its own object directory (csrc/<name>/build/),
stamp and resources JSON, its C ABI in include/isochrones_amd_<name>.h.  The same gates as build.py apply: no AGPRs, scratch
within the spec's budget (resources.violations), at most max_vgpr VGPRs and at least min_waves waves per SIMD for every kernel,
and a clean isa_check scan of the generated code."""
from __future__ import annotations

import concurrent.futures
import dataclasses
import glob
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(HERE, "..", "..", "include")


class LibraryBuildError(RuntimeError):
    """A kernel of a side library outside the budget, or a compile / link failure."""


@dataclasses.dataclass(frozen=True)
class KernelLibrary:
    """What differs between the side libraries; its repr is part of the digest, so editing a field rebuilds that library."""
    name: str
    flags: tuple
    #: every kernel the library compiles (its tests pin this set)
    kernels: tuple
    max_vgpr: int
    min_waves: int
    #: (kernel family, bytes of scratch per lane it may use) pairs; every other kernel none
    scratch_budget: tuple = ()
    #: headers outside csrc/<name>/ that the sources include, relative to csrc/: file names (a missing one is an error) and
    #: patterns with a *
    extra_headers: tuple = ()
    #: removed from the kernel names of the resource table
    strip_prefix: str = ""

    # the names the build scripts of the libraries had as module attributes
    SRC = property(lambda self: os.path.join(HERE, self.name))
    OUT = property(lambda self: os.path.join(HERE, "libiso_%s.so" % self.name))
    OBJDIR = property(lambda self: os.path.join(self.SRC, "build"))
    STAMP = property(lambda self: os.path.join(HERE, "libiso_%s.stamp" % self.name))
    RESOURCES = property(lambda self: os.path.join(HERE, "libiso_%s.resources.json" % self.name))
    HEADER = property(lambda self: os.path.join(INCLUDE, "isochrones_amd_%s.h" % self.name))
    FLAGS = property(lambda self: list(self.flags))
    KERNELS = property(lambda self: self.kernels)
    MAX_VGPR = property(lambda self: self.max_vgpr)
    MIN_WAVES = property(lambda self: self.min_waves)
    #: (0 when no family has a budget, which is how the libraries without one spelled it)
    SCRATCH_BUDGET = property(lambda self: dict(self.scratch_budget) or 0)

    def sources(self):
        return sorted(glob.glob(os.path.join(self.SRC, "*.hip")))

    def headers(self):
        extra = [h for pat in self.extra_headers
                 for h in (sorted(glob.glob(os.path.join(HERE, pat))) if "*" in pat else [os.path.join(HERE, pat)])]
        return [self.HEADER] + sorted(glob.glob(os.path.join(self.SRC, "*.h"))) + extra

    def source_digest(self) -> str:
        from .build import compiler_version
        h = hashlib.sha256((compiler_version() + repr(self)).encode())
        for path in self.sources() + self.headers() + [os.path.abspath(__file__), os.path.join(HERE, "resources.py"),
                                                       os.path.join(HERE, "isa_check.py")]:
            h.update(os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as f:
                h.update(f.read())
        return h.hexdigest()

    def up_to_date(self) -> bool:
        from .build import file_sha256
        try:
            src, so = open(self.STAMP).read().split()[:2]
        except (OSError, ValueError):
            return False
        return (os.path.exists(self.OUT) and os.path.exists(self.RESOURCES) and src == self.source_digest()
                and so == file_sha256(self.OUT))

    def resource_table(self) -> dict:
        with open(self.RESOURCES) as f:
            return json.load(f)

    def violations(self, table: dict) -> list:
        from . import resources as R
        bad = R.violations(table, scratch_budget=dict(self.scratch_budget), default_scratch=0, max_agpr=0)
        for name, r in sorted(table.items()):
            if r.get("vgpr", 0) > self.max_vgpr:
                bad.append("%s: %d VGPRs (limit %d)" % (name, r["vgpr"], self.max_vgpr))
            if r.get("waves", 0) < self.min_waves:
                bad.append("%s: %d waves per SIMD (at least %d)" % (name, r.get("waves", 0), self.min_waves))
        return bad

    def build(self, force: bool = False, verbose: bool = False) -> str:
        """Compile, gate and link when the sources changed; return the library path."""
        from . import resources as R
        from . import isa_check as I
        from .build import hipcc, file_sha256
        digest = self.source_digest()
        if not force and self.up_to_date():
            return self.OUT
        os.makedirs(self.OBJDIR, exist_ok=True)
        cc = hipcc()
        objs, table = [], {}

        def compile_one(src):
            obj = os.path.join(self.OBJDIR, os.path.basename(src)[:-4] + ".o")
            p = subprocess.run([cc] + self.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj],
                               cwd=self.SRC, stderr=subprocess.PIPE, text=True, errors="replace")
            return src, obj, p

        jobs = max(1, min(int(os.environ.get("MAX_JOBS") or 8), len(self.sources())))
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            done = list(pool.map(compile_one, self.sources()))
        for src, obj, p in done:
            rest = [ln for ln in p.stderr.splitlines() if "kernel-resource-usage" not in ln and not R.is_remark_context(ln)]
            if verbose or p.returncode != 0 or any("warning:" in ln or "error:" in ln for ln in rest):
                sys.stderr.write("\n".join(rest) + ("\n" if rest else ""))
            if p.returncode != 0:
                raise LibraryBuildError("hipcc failed on %s" % os.path.basename(src))
            with open(obj[:-2] + ".res", "w") as f:
                f.write(p.stderr)
            table.update({k.replace(self.strip_prefix, ""): v for k, v in R.parse(p.stderr).items()})
            objs.append(obj)
        for stale in (self.STAMP, self.RESOURCES):
            try:
                os.remove(stale)
            except OSError:
                pass
        bad = self.violations(table)
        if bad:
            raise LibraryBuildError("kernel(s) of %s outside the budget:\n  " % os.path.basename(self.OUT) + "\n  ".join(bad))
        faults = [tuple(x) for obj in objs for x in I.scan_library(obj, jobs=1)]
        if faults:
            raise I.IsaFault(I.render(faults))
        subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", self.OUT] + objs, cwd=self.SRC)
        with open(self.RESOURCES, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
        with open(self.STAMP, "w") as f:
            f.write(digest + "\n" + file_sha256(self.OUT) + "\n")
        return self.OUT
