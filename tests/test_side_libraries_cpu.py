"""The shared builder (csrc/sidelib.py), the six specs (csrc/libraries.py) and the shared loader (_sidelib.py) of the side
libraries, without building or loading any of them: the libraries keep apart from each other and from libiso_hip.so, a
spec's digest follows what it is built from and nothing else, the gates report each kind of violation, the loader's errors."""
import dataclasses
import itertools
import os
import re
import shutil
import types

import pytest

from isochrones_amd.csrc import build as main
from isochrones_amd.csrc import libraries, sidelib
from isochrones_amd.csrc.libraries import ALL, DERIVED, NESTED, SOLVE


def test_the_libraries_do_not_touch_each_other():
    assert [s.name for s in ALL] == ["cluster", "nested", "solve", "diag", "derived", "predict"]
    assert ALL == (libraries.CLUSTER, NESTED, SOLVE, libraries.DIAG, DERIVED, libraries.PREDICT)
    for a, b in itertools.combinations((main,) + ALL, 2):
        assert a.OUT != b.OUT and a.OBJDIR != b.OBJDIR and a.STAMP != b.STAMP and a.RESOURCES != b.RESOURCES
        assert a.sources() and b.sources() and not set(a.sources()) & set(b.sources())
    for spec in ALL:
        assert not any(spec.name in os.path.basename(s) for s in main.sources())
        assert os.path.exists(spec.HEADER) and spec.HEADER in spec.headers()
    assert set(DERIVED.KERNELS) == {"k_derived_chain"}


def test_digest_follows_the_spec_the_flags_and_the_headers(tmp_path, monkeypatch):
    base = DERIVED.source_digest()
    assert base == DERIVED.source_digest() == dataclasses.replace(DERIVED).source_digest()
    assert dataclasses.replace(DERIVED, max_vgpr=DERIVED.max_vgpr - 1).source_digest() != base
    assert dataclasses.replace(DERIVED, flags=DERIVED.flags + ("-DX",)).source_digest() != base
    assert dataclasses.replace(DERIVED, flags=DERIVED.flags[:-1]).source_digest() != base
    # a header: a copy of the library's own, listed as an extra one
    copy = str(tmp_path / os.path.basename(DERIVED.HEADER))
    shutil.copyfile(DERIVED.HEADER, copy)
    spec = dataclasses.replace(DERIVED, extra_headers=(copy,))
    assert spec.headers()[-1] == copy
    before = spec.source_digest()
    with open(copy, "r+b") as f:
        byte = f.read(1)
        f.seek(0)
        f.write(bytes([byte[0] ^ 1]))
    assert spec.source_digest() != before
    assert len({s.source_digest() for s in ALL}) == len(ALL)
    # the files it reads: the builder and the gates, not the file of specs (another library's spec is no part of it)
    read = []
    monkeypatch.setattr(sidelib, "open", lambda path, *a: read.append(os.path.basename(path)) or open(path, *a), raising=False)
    assert DERIVED.source_digest() == base
    assert set(read) == {os.path.basename(p) for p in DERIVED.sources() + DERIVED.headers()} | {"sidelib.py", "resources.py",
                                                                                                 "isa_check.py"}
    assert "libraries.py" not in read and len(read) == len(set(read))


def test_nested_digest_covers_the_main_library_headers_it_includes():
    names = [os.path.basename(h) for h in NESTED.headers()]
    assert names[0] == "isochrones_amd_nested.h"
    assert {"iso_fast_kernel.h", "iso_internal.h", "isochrones_amd.h"} <= set(names)
    fast = [h for h in NESTED.headers() if os.path.basename(os.path.dirname(h)) == "fast"]
    assert fast and all(os.path.exists(h) for h in NESTED.headers())
    assert all(os.path.basename(os.path.dirname(h)) in ("include", "solve", "common") for h in SOLVE.headers())
    # a header named outright is not searched for: one that is not there stops the digest instead of dropping out of it
    gone = dataclasses.replace(SOLVE, extra_headers=("iso_no_such_header.h",))
    assert os.path.basename(gone.headers()[-1]) == "iso_no_such_header.h"
    with pytest.raises(OSError):
        gone.source_digest()
    assert dataclasses.replace(SOLVE, extra_headers=SOLVE.extra_headers + ("no_such_dir/*.h",)).headers() == SOLVE.headers()


def _reached_headers(spec):
    """Every file a quoted #include of the spec's sources reaches: looked up next to the including file, then in include/
    (the -I of every spec), and followed on through the library's own directory, csrc/common/ and include/."""
    followed = {os.path.realpath(d) for d in (spec.SRC, os.path.join(sidelib.HERE, "common"), sidelib.INCLUDE)}
    seen, todo = set(), list(spec.sources())
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
    return seen


@pytest.mark.parametrize("spec", libraries.BUILD_ORDER + libraries.ADDED + libraries.NEWER, ids=lambda s: s.name)
def test_the_digest_covers_every_header_the_sources_reach(spec):
    """A header that is reached but not listed would not rebuild the library when it is edited."""
    listed = {os.path.realpath(h) for h in spec.headers()}
    missing = sorted(os.path.relpath(h, sidelib.HERE) for h in _reached_headers(spec) - listed)
    assert not missing, (spec.name, missing)
    if spec in (libraries.HIER,) + libraries.NEWER:
        assert any(h.endswith("family_lnf.h") for h in listed) and any(h.endswith("wave_reduce.h") for h in listed)


def test_the_population_libraries_keep_no_copies_of_what_they_share():
    """hier, select, reweight, relation and binned: the family arithmetic, the wavefront reductions and the column view live in
    csrc/common/ alone, and the three row-total kernels are one body."""
    for spec in (libraries.HIER,) + libraries.NEWER:
        (path,) = spec.sources()
        src = open(path).read()
        for gone in ("__shfl_xor", "struct DevCol", "feh_shape"):
            assert gone not in src, (spec.name, gone)
    assert [s.name for s in (libraries.HIER,) + libraries.NEWER] == ["hier", "select", "reweight", "relation", "binned"]
    for name in ("hier", "relation", "binned"):
        src = open(os.path.join(sidelib.HERE, name, name + ".hip")).read()
        (body,) = re.findall(r"__global__[^{;]*\bk_%s_total\s*\([^)]*\)\s*\{(.*?)\n\}" % name, src, re.S)
        assert len(body.strip().splitlines()) <= 3 and "row_total(" in body, (name, body)
    block = open(os.path.join(sidelib.HERE, "common", "hier_block.h")).read()
    assert block.count("void row_total(") == 1 and "__forceinline__ void row_total(" in block


def _row(**kw):
    return dict(dict(agpr=0, scratch=0, vgpr=40, waves=8, sgpr=10, lds=0, vgpr_spill=0, sgpr_spill=0), **kw)


def test_violations_name_the_kernel_and_the_limit():
    assert DERIVED.violations({"k_fine": _row(vgpr=DERIVED.max_vgpr, waves=DERIVED.min_waves)}) == []
    for bad in (dict(agpr=4), dict(scratch=8), dict(vgpr=DERIVED.max_vgpr + 1), dict(waves=DERIVED.min_waves - 1)):
        got = DERIVED.violations({"k_fine": _row(), "k_bad": _row(**bad)})
        assert len(got) == 1 and got[0].startswith("k_bad"), (bad, got)
    assert len(DERIVED.violations({"k": _row(agpr=1, scratch=16, vgpr=300, waves=1)})) == 4


def test_scratch_budget_is_per_family():
    assert NESTED.SCRATCH_BUDGET == {"k_catalog_nested": 148} and DERIVED.SCRATCH_BUDGET == 0 == SOLVE.SCRATCH_BUDGET
    assert len({hash(s) for s in ALL}) == len(ALL)                          # frozen all the way down
    name = NESTED.KERNELS[-1]
    assert name == "k_catalog_nested<1, 3, 12>"
    assert NESTED.violations({name: _row(vgpr=256, waves=2, scratch=148)}) == []
    got = NESTED.violations({name: _row(vgpr=256, waves=2, scratch=149)})
    assert len(got) == 1 and got[0].startswith(name)
    assert len(NESTED.violations({"k_other": _row(scratch=8)})) == 1        # the budget is that family's alone
    assert len(SOLVE.violations({name: _row(scratch=8)})) == 1             # and that library's alone


def test_loader_errors(tmp_path):
    from isochrones_amd._cabi import IsoError
    from isochrones_amd._sidelib import SideLibrary
    missing = str(tmp_path / "libiso_absent.so")
    side = SideLibrary("absent", "absent-minded", lambda L: None, path=missing)
    assert side.library_path() == missing
    with pytest.raises(IsoError) as e:
        side.lib()
    assert missing in str(e.value) and "absent-minded library not found" in str(e.value) and "no CPU fallback" in str(e.value)
    side._lib = types.SimpleNamespace(iso_absent_last_error=lambda: b"what went wrong")     # stands in for a loaded library
    side.check(0)
    with pytest.raises(IsoError) as e:
        side.check(-1)
    assert e.value.rc == -1 and "absent C-ABI error -1: what went wrong" in str(e.value)
    for cabi in ("cluster", "nested", "solve", "diag", "derived", "predict"):
        mod = __import__("isochrones_amd._%s_cabi" % cabi, fromlist=["x"])
        assert mod.library_path() == os.path.join(os.path.dirname(main.HERE), "csrc", "libiso_%s.so" % cabi)
        assert mod.EXPORTED_SYMBOLS[:2] == ("iso_%s_version" % cabi, "iso_%s_last_error" % cabi)
