"""The side libraries, each a spec for sidelib.KernelLibrary, in the order __graft_entry__.build() builds them
(BUILD_ORDER + ADDED + NEWER + LATEST).

    python -m isochrones_amd.csrc.libraries NAME [--force] [--verbose]

A new library is one more spec here (and its name in LATEST), its sources in csrc/<name>/ and its header
include/isochrones_amd_<name>.h."""
from __future__ import annotations

import sys

from .sidelib import INCLUDE, KernelLibrary

_COMMON = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math")
#: what every library but NESTED is built with.  -ffp-contract=off: the compiler fuses no multiply-add on its own (each spec says
#: what that buys)
_NO_CONTRACT = _COMMON + ("-ffp-contract=off", "-Wall", "-Wno-unused-function", "-I" + INCLUDE)

# the star-cluster likelihood (csrc/cluster/)
# -ffp-contract=off: every product and sum is rounded as written, in the reference's order (no fused multiply-adds), so that
# the kernel's cells follow the reference's arithmetic as closely as its libm calls allow
CLUSTER = KernelLibrary(
    name="cluster", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_cluster_library.py pins this set)
    kernels=("k_cluster_finish", "k_cluster_pairs"),
    max_vgpr=256, min_waves=2, extra_headers=("common/last_error.h",))

# nested sampling of a catalog (csrc/nested/).  Its kernels include libiso_hip.so's header-only device code
# (iso_fast_kernel.h: lnpost_wave and what it needs), so those headers are part of its source digest.
# (the flags libiso_hip.so's fused kernels are built with: lnpost_wave is the same code here and there)
#: (parametrisation, stars per system) of every kernel family; each has the instantiations for 1 .. 12 bands
_NESTED_FAMILIES = ((0, 1), (1, 1), (1, 2), (1, 3))
NESTED = KernelLibrary(
    name="nested",
    flags=_COMMON + ("-Wall", "-Wno-unused-function", "-Wno-bitwise-instead-of-logical", "-mllvm", "-disable-machine-licm",
                     "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-I" + INCLUDE),
    #: every kernel the library compiles (tests/test_nested_catalog_cpu.py pins this set)
    kernels=tuple("k_catalog_nested<%d, %d, %d>" % (kind, ns, nb) for kind, ns in _NESTED_FAMILIES for nb in range(1, 13)),
    #: bytes of scratch per lane the family may use, as k_catalog_start has a budget in resources.py: a ratchet, set to what
    #: the worst instantiation needs today.  A workgroup here owns a CU's LDS, so one wave per SIMD runs whatever the registers
    #: say and the kernel is compiled for 256 VGPRs; at that size only the many-band multiples spill (binary, 12 bands: 8 B;
    #: triple, 10 / 11 / 12 bands: 8 / 68 / 148 B), every other instantiation nothing.
    scratch_budget=(("k_catalog_nested", 148),),
    max_vgpr=256, min_waves=2,
    extra_headers=("iso_fast_kernel.h", "iso_internal.h", "../../include/isochrones_amd.h", "fast/*.h"),
    strip_prefix="nestk::")

# the exact (mass, age, [Fe/H]) -> EEP solve (csrc/solve/)
# -ffp-contract=off: every product and sum is rounded as written (no fused multiply-adds), so that g(k) is the interpolator's
# value bit for bit and stays nondecreasing in k, which the bisection rests on
SOLVE = KernelLibrary(
    name="solve", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_solve_library.py pins this set)
    kernels=("k_solve_last_axis",),
    #: the kernel is a chain of dependent gathers: its throughput is occupancy, so the register budget is the 8-waves-per-SIMD
    #: one, 64 VGPRs; the wave gate itself is the two per SIMD every library has at least
    max_vgpr=64, min_waves=2, extra_headers=("common/grid_cell.h", "common/last_error.h"))

#: shared by the libraries that post-process a stored chain (internal; named outright: a missing one stops the digest)
_CHAIN_HEADERS = ("common/grid_cell.h", "common/chain_view.h", "common/last_error.h")
#: the same for the two that interpolate grid cells along it (grid_interp.h: the cell the population library shares)
_CELL_HEADERS = _CHAIN_HEADERS + ("common/grid_interp.h",)
#: shared by HIER and the four libraries on its records: the family arithmetic (family_lnf.h, its only home) and the
#: wavefront reductions.  Every spec names every header its sources reach, directly or through another header: one that is
#: not named is not in the source digest (tests/test_side_libraries_cpu.py follows the #include lines)
_HIER_HEADERS = ("common/family_lnf.h", "common/grid_cell.h", "common/last_error.h", "common/wave_reduce.h")
#: the same for the four that are not HIER, whose own header isochrones_amd_hier.h is
_RECORD_HEADERS = ("../../include/isochrones_amd_hier.h",) + _HIER_HEADERS
#: an iso_hier_column as the kernels read it (hier_columns.h), for the libraries that read stored chains through one
_COLUMN_HEADERS = ("common/hier_columns.h", "common/chain_view.h")
#: the entry points HIER and RELATION share (hier_lnlike.h) and the row total they share with BINNED (hier_block.h)
_LNLIKE_HEADERS = _COLUMN_HEADERS + ("common/hier_block.h", "common/hier_lnlike.h")

# per-star chain convergence diagnostics (csrc/diag/)
# -ffp-contract=off: the compiler fuses nothing on its own; the kernel's fused multiply-adds are the ones written as fma(),
# which is part of the documented summation order (a pair's row is bit-identical alone or in any batch)
DIAG = KernelLibrary(
    name="diag", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_diag_library.py pins this set)
    kernels=("k_diag_chain",),
    #: k_diag_chain compiles to 44 VGPRs, no scratch and 8 waves per SIMD.  Its inner loop is two LDS reads per multiply-add,
    #: hidden by the other wavefronts of the CU, so the budget is the 8-waves-per-SIMD one: 64 VGPRs, and no scratch at all
    max_vgpr=64, min_waves=8, extra_headers=_CHAIN_HEADERS + ("common/wave_reduce.h",))

# model-grid columns along a stored chain (csrc/derived/)
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a sample's values are bit-identical in any batch, ensemble range and layout)
DERIVED = KernelLibrary(
    name="derived", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_derived_library.py pins this set)
    kernels=("k_derived_chain",),
    #: k_derived_chain compiles to 120 VGPRs, no scratch and 4 waves per SIMD: the eight-column branch keeps 8 accumulators and
    #: the cell's corner loads in flight (16 two-double loads a sample; they are what hides the gather latency).  Forcing 8 waves
    #: (64 VGPRs) spills to scratch, so the budget is the 4-waves-per-SIMD one: 128 VGPRs, and no scratch at all
    max_vgpr=128, min_waves=4, extra_headers=_CELL_HEADERS)

# the posterior-predictive check of a stored chain (csrc/predict/)
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a sample's values are bit-identical in any batch, ensemble range and layout)
PREDICT = KernelLibrary(
    name="predict", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_predict_library.py pins this set)
    kernels=("k_predict_chain",),
    #: k_predict_chain compiles to 242 VGPRs, no scratch and 2 waves per SIMD.  A sample holds the brackets and weights of a 4-D
    #: cell, eight band accumulators, four corners of eight bands in flight and the model cell's 32 values; the call's 60-odd
    #: uniform values (two tables, strides, outputs) are staged in LDS because as kernel arguments they overflow the SGPR file and
    #: their spill slots count as scratch.  The workgroup is two waves, so the budget is the 2-waves-per-SIMD one: 256 VGPRs
    max_vgpr=256, min_waves=2, extra_headers=_CELL_HEADERS)

# a batch of coeval single or binary systems evaluated on the model and the BC grid (csrc/population/)
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a system's values are bit-identical alone and in any batch)
POPULATION = KernelLibrary(
    name="population", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_population_library.py pins this set)
    kernels=("k_population_eval",),
    #: k_population_eval compiles to 246 VGPRs, no scratch, 32 KB of LDS and 2 waves per SIMD.  A system holds the model
    #: cell's eight weights, eight column accumulators and their corner loads in flight (k_derived_chain's pressure), then
    #: the (Teff, logg, feh, Mbol) of two components, two sets of eight band accumulators (at AV and at AV = 0), their
    #: corner loads and a binary's two sets of eight sums (k_predict_chain's pressure, doubled by the second lookup).  Held to
    #: 4 waves (128 VGPRs) it spills 190 registers to scratch, with four bands a pass still 94; so the budget is the
    #: 2-waves-per-SIMD one: 256 VGPRs, and no scratch at all.  Its uniform arguments (two tables, eight pointers) overflow
    #: the SGPR file into VGPR lanes, not into scratch, so they are not staged in LDS as k_predict_chain's are
    max_vgpr=256, min_waves=2, extra_headers=("common/grid_cell.h", "common/grid_interp.h", "common/last_error.h"))

# the hierarchical (population) likelihood from the stored chains of a catalog (csrc/hier/)
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a star's row is bit-identical alone, in any batch and in any tiling of the hyper rows)
HIER = KernelLibrary(
    name="hier", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_hier_library.py pins this set)
    kernels=("k_hier_stars", "k_hier_total"),
    #: k_hier_stars compiles to 153 VGPRs, no scratch, 3.3 KB of LDS and 3 waves per SIMD.  A lane holds the maximum, sum w and
    #: sum w^2 of the tile's eight rows (48 registers), the sample's eight log ratios (16) and the temporaries of eight
    #: inlined family evaluations, the FEH one with three exp and a log in flight.  Held to 4 waves (128 VGPRs) it spills 45
    #: registers to scratch; the per-(row, sample) exp binds, not latency, so the budget is the 3-waves-per-SIMD one: 168
    #: VGPRs, and no scratch at all.  k_hier_total is 17 VGPRs at 8 waves
    max_vgpr=168, min_waves=3, extra_headers=_HIER_HEADERS + _LNLIKE_HEADERS)

# the detectable fraction of a population density from an injection set (csrc/select/): the selection term of HIER's
# likelihood.  It reads HIER's records (its header includes isochrones_amd_hier.h) and evaluates them through
# common/family_lnf.h, the family arithmetic HIER itself compiles
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a row is bit-identical alone, in any tiling of the hyper rows and on every call)
SELECT = KernelLibrary(
    name="select", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_select_library.py pins this set)
    kernels=("k_select_partial", "k_select_total"),
    #: k_select_partial is k_hier_stars's loop over a chunk of injections instead of a star's samples: 152 VGPRs, no
    #: scratch, 3.1 KB of LDS and 3 waves per SIMD, for the same reason (the accumulators of eight rows, eight inlined
    #: family evaluations); the budget is the 3-waves-per-SIMD one: 168 VGPRs, and no scratch at all.  k_select_total is
    #: 44 VGPRs at 8 waves
    max_vgpr=168, min_waves=3, extra_headers=_RECORD_HEADERS)

# the population-informed posterior of every star from its stored chain (csrc/reweight/): per-sample weights under the hyper
# rows of a fitted population, and weighted per-star summaries.  It reads HIER's records and columns (its header includes
# isochrones_amd_hier.h), evaluates them through common/family_lnf.h and takes HIER's ell as the weights' normaliser
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a star's outputs are bit-identical alone, in any batch, star range and layout)
REWEIGHT = KernelLibrary(
    name="reweight", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_reweight_library.py pins this set)
    kernels=("k_reweight_summary", "k_reweight_weights"),
    #: k_reweight_weights compiles to 101 VGPRs, no scratch, 19 KB of LDS (a tile of 64 rows' records) and 4 waves per SIMD.
    #: A lane holds the sample's four columns with their logs and interim terms (24 registers) and one inlined family
    #: evaluation, the FEH one with three exp and a log in flight; the rows run innermost into one accumulator, so
    #: k_hier_stars's 48 registers of per-row sums are gone.  The column index is a run-time loop over select chains: unrolled,
    #: its four independent family evaluations interleave to 232 VGPRs (2 waves).  Its 49 spilled SGPRs (the argument block)
    #: go to VGPR lanes, not to scratch.  Held to 5 waves (96 VGPRs) it spills 2 registers to scratch; the per-(row, sample)
    #: exp binds, not latency, so the budget is the 4-waves-per-SIMD one: 128 VGPRs, and no scratch at all.
    #: k_reweight_summary (16 bins of a radix pass in registers) is 59 VGPRs at 8 waves
    max_vgpr=128, min_waves=4, extra_headers=_RECORD_HEADERS + _COLUMN_HEADERS)

# HIER's likelihood for a population density that links columns (csrc/relation/): a column's Gaussian follows another column
# linearly, so its truncation normaliser is per (hyper row, sample) and is evaluated in the kernel.  It reads HIER's records
# and columns (its header includes isochrones_amd_hier.h) and evaluates the kinds 1 .. 8 through common/family_lnf.h, the
# linked kind through common/relation_lnf.h
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a star's row is bit-identical alone, in any batch and in any tiling of the hyper rows,
# and equal to HIER's where no record is linked)
RELATION = KernelLibrary(
    name="relation", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_relation_library.py pins this set)
    kernels=("k_relation_stars", "k_relation_total"),
    #: k_relation_stars compiles to 205 VGPRs, no scratch, 3.4 KB of LDS and 2 waves per SIMD: k_hier_stars's 153 (the sums of
    #: eight rows, eight inlined family evaluations) and on top the sample's four values, kept for the parents, and the linked
    #: term with two erfc and a log in flight.  A row tile of 4 compiles to 165 VGPRs and 3 waves and was measured slower (72.9
    #: against 68.3 ms): the per-sample work is shared by half as many rows.  So the budget is the
    #: 2-waves-per-SIMD one: 256 VGPRs, and no scratch at all.  Its 43 spilled SGPRs (the argument block) go to VGPR lanes, not
    #: to scratch.  k_relation_total is k_hier_total: 17 VGPRs at 8 waves
    max_vgpr=256, min_waves=2, extra_headers=_RECORD_HEADERS + ("common/relation_lnf.h",) + _LNLIKE_HEADERS)

# HIER's likelihood for a population density that is piecewise constant on a grid of bins over one or two columns
# (csrc/binned/): a histogram's mean weight is linear in the cell heights, so the chain is compressed once to a table of B
# numbers per star and every likelihood evaluation is a contraction of that table with the rows' heights.  It reads HIER's
# records and columns (its header includes isochrones_amd_hier.h) and evaluates the kinds 1 .. 8 through common/family_lnf.h
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a star's table is bit-identical alone, in any batch, star range and layout, a (row, star)
# result in any tiling of the hyper rows)
BINNED = KernelLibrary(
    name="binned", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_binned_library.py pins this set)
    kernels=("k_binned_compress", "k_binned_rows", "k_binned_total"),
    #: k_binned_compress compiles to 91 VGPRs, no scratch, 4.4 KB of LDS (a tile's 256 weights and cells, the edges, the
    #: records) and 5 waves per SIMD.  A lane holds one sample at a time: a column's value, its log and interim term, one
    #: inlined family evaluation (the FEH one with three exp and a log in flight) and the bracket search; the cell's two sums
    #: are two registers, since a lane owns one cell.  The column index is a run-time loop, as in k_reweight_weights.  Its 24
    #: spilled SGPRs (the argument block) go to VGPR lanes, not to scratch.  The kernel runs once per (catalog, edges), so the
    #: budget is what it compiles to, the 5-waves-per-SIMD one: 96 VGPRs, and no scratch at all.  k_binned_rows (the sums of
    #: eight rows, 32 registers, and one cell's two loads) is 55 VGPRs at 8 waves with 8.1 KB of LDS (the tile's u and u * u),
    #: and 64 with the header's rescue behind it (a rare per-lane tail with an exp and a log), held at 8 waves by
    #: amdgpu_waves_per_eu(8, 8) without scratch;
    #: k_binned_total is k_hier_total: 17 VGPRs at 8 waves
    max_vgpr=96, min_waves=5, extra_headers=_RECORD_HEADERS + _COLUMN_HEADERS + ("common/hier_block.h",))

# the per-star counterpart of BINNED (csrc/shrink/): every star's weights and bin memberships once a fitted histogram
# replaces the interim prior.  The sum over the hyper rows belongs to the (star, cell), so it is taken once from BINNED's
# tables, and the chain is read once with one exp per sample whatever the number of rows.  It reads HIER's records and
# columns and BINNED's constants (its header includes both) and evaluates the per-sample term through
# common/binned_sample.h, a restatement of binned.hip's (BINNED's header list is pinned; moving it over is the follow-up)
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a star's outputs are bit-identical alone, in any batch, star range and layout, a (star,
# cell) result in any block of stars and any tile of cells)
SHRINK = KernelLibrary(
    name="shrink", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_shrink_library.py pins this set)
    kernels=("k_shrink_cells", "k_shrink_weights"),
    #: k_shrink_weights compiles to 82 VGPRs, no scratch, 1.9 KB of LDS (the records, the edges, the star's lnG) and 5 waves per
    #: SIMD: k_binned_compress's per-sample work (one column at a time, one inlined family evaluation, the bracket search)
    #: with one exp on top and without the second pass's tile.  Its 10 spilled SGPRs (the argument block) go to VGPR lanes, not
    #: to scratch.  The budget is what it compiles to, the 5-waves-per-SIMD one: 96 VGPRs, and no scratch at all.
    #: k_shrink_cells is 62 VGPRs at 8 waves with 8 KB of LDS, at a tile of 2 cells.  The compiler hoists the constants of exp
    #: and log to the kernel's top, 30 VGPRs that stay live throughout, so a tile's maxima and sums next to them decide the
    #: occupancy: with a tile of 8 in registers it is 95 VGPRs (5 waves), with 4 in registers 78 (6 waves), with 4 parked in
    #: LDS between the passes 69 (7 waves); held to 64 VGPRs those spill 124, 60 and 12 bytes to scratch.  The tile only
    #: sets how often ell is read again (B / 2 times two passes), next to one exp per (row, cell)
    max_vgpr=96, min_waves=5,
    extra_headers=("../../include/isochrones_amd_binned.h",) + _RECORD_HEADERS + _COLUMN_HEADERS + ("common/binned_sample.h",))

# random draws of synthetic populations and injection sets (csrc/draw/): every column of every system from counter-based
# uniforms (Philox4x32-10, common/philox.h) through an exact inverse distribution function (ndtri: common/ndtri.h).  It
# shares no record with the other libraries: a draw record carries the thresholds of an inverse, not a log density
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a system's draws are bit-identical alone, in any batch, at any first and through index)
DRAW = KernelLibrary(
    name="draw", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_draw_library.py pins this set)
    kernels=("k_draw_systems",),
    #: k_draw_systems compiles to 127 VGPRs, no scratch, no LDS and 4 waves per SIMD, asked for by its launch bounds.  Left
    #: alone the compiler takes 185 VGPRs (2 waves): it interleaves the ten Philox rounds with the constants of erfc, exp,
    #: log1p and ndtri's three rational functions, all inlined into one loop body, and none of that needs to be live at once.
    #: A lane holds the system's eight values (16 registers), the two uniforms and one inverse at a time.  The kernel writes
    #: 8 bytes per (system, column) next to some hundred integer and float64 operations, with no load to wait for, so the
    #: waves only have to cover the arithmetic's own latency; the budget is the 4-waves-per-SIMD one: 128 VGPRs, and no scratch
    #: at all.  Its 17 spilled SGPRs (a record of the argument block) go to VGPR lanes, not to scratch
    max_vgpr=128, min_waves=4, extra_headers=("common/last_error.h", "common/ndtri.h", "common/philox.h"))

# the moments of the stars' posterior cell probabilities under a binned population (csrc/binfit/): the expected number of
# stars per cell and the sum of the outer products, per hyper row, from BINNED's per-star tables alone: the E-step of a
# maximum-likelihood fit of the cell heights, the gradient and the curvature of BINNED's ln L.  It reads no record and no
# chain; its header includes BINNED's for the limit of a grid
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a row's outputs are bit-identical alone, in any sub-range of the rows and on every call)
BINFIT = KernelLibrary(
    name="binfit", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_binfit_library.py pins this set)
    kernels=("k_binfit_partial", "k_binfit_total"),
    #: k_binfit_partial compiles to 124 VGPRs (120 before the header's rescue), no scratch, 33.5 KB of LDS and 4 waves per SIMD.  A lane holds the sums of its
    #: block of 3 x 3 pairs and of its cell (20 registers), the six places of the block's cells in a tile row, the sixteen
    #: loads of its star's cells that a tile issues together (32, with their addresses) and, in the walk unrolled over two
    #: stars, their twelve 64-bit LDS reads in flight (24).  The waves are set by the LDS, not by the registers: a tile of
    #: 64 stars x 65 doubles lets four workgroups share a CU's 160 KB, which is four waves per SIMD, and at that occupancy a
    #: lane may use 128 registers.  Carrying the next tile's sixteen values through the walk (a prefetch a tile ahead) takes
    #: 138 to 152 registers, 3 waves, and held to 128 it spills 8 bytes to scratch: left out.  The budget is the
    #: 4-waves-per-SIMD one: 128 VGPRs, and no scratch at all.
    #: k_binfit_total (a running sum and the addresses of its two stores) is 14 VGPRs at 8 waves
    max_vgpr=128, min_waves=4,
    extra_headers=("../../include/isochrones_amd_binned.h", "../../include/isochrones_amd_hier.h", "common/last_error.h"))

# a batch of weighted EM fits of a binned population's cell masses, and the star weights of a bootstrap (csrc/emfit/): one
# workgroup per replicate iterates masses <- N / sum N on BINNED's per-star tables with the whole loop inside the kernel, so
# R bootstrap replicates cost no host round trip per step.  It reads no record and no chain; its header includes BINNED's for
# the limit of a grid, and the weights come from common/philox.h
# -ffp-contract=off: the compiler fuses nothing, and the sources write no fma(): every product and every sum of the header's
# definition is rounded on its own (a replicate's outputs are bit-identical alone, in any batch, at any replicate offset, in
# any chain of launches and on every call)
EMFIT = KernelLibrary(
    name="emfit", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_emfit_library.py pins this set)
    kernels=("k_emfit_run<8>", "k_emfit_run<16>", "k_emfit_run<32>", "k_emfit_run<64>", "k_emfit_weights"),
    #: k_emfit_run<64> compiles to 220 VGPRs, no scratch, no spill, 3.9 KB of LDS and 2 waves per SIMD; <32> to 157 (3 waves),
    #: <16> to 122 and <8> to 106 (4); before the header's rescue 208, 144, 110 and 100 with 3.7 KB.  A lane holds one sum per cell of the padded grid (2 BP registers: 128 at 64 cells), the
    #: star's Q, W and live sums, the eight loads a pass has in flight with their addresses, and an inlined log and division.
    #: Left alone the compiler lifts the BP heights of the second pass and the BP comparisons with B out of the star loop
    #: (254 VGPRs, 260 B of scratch and 107 spilled SGPRs at 64 cells): above 16 cells the heights are read from LDS per
    #: star, as in the first pass, and B is compared as a scalar where it is used.  With one load waited for at a time
    #: the second pass was the kernel's latency (192 VGPRs, 519 us an evaluation of 10^4 stars x 64 cells); eight a group
    #: cost 16 registers and took it to 230 us.  One workgroup runs a replicate whatever its occupancy and a batch of R
    #: replicates fills R CUs, so the second wave per SIMD only hides the loads of another replicate on the same CU
    #: (R > 256); the budget is the 2-waves-per-SIMD one: 256 VGPRs, and no scratch at all.  k_emfit_weights (ten Philox
    #: rounds, eighteen comparisons or one log) is 19 VGPRs at 8 waves
    max_vgpr=256, min_waves=2,
    extra_headers=("../../include/isochrones_amd_binned.h", "../../include/isochrones_amd_hier.h", "common/last_error.h",
                   "common/philox.h", "common/wave_reduce.h"))

# per-star moments of the star-cluster likelihood's integrand (csrc/members/): what a cluster fit says about each member
# star.  k_cluster_pairs's plan with six running trapezoids a lane instead of one, and an outer pass that turns them into
# ln like_s and eleven moments.  It shares no source with CLUSTER (whose header list and kernel set are pinned): the cell
# arithmetic is restated, and ln_like being the same bits as CLUSTER's lnlike_star is what its GPU test holds the two to
# -ffp-contract=off: every product and sum is rounded as written (no fused multiply-adds), which that bit identity and
# the header's summation order rest on (a (row, star) result is bit-identical alone, in any batch and on every call)
MEMBERS = KernelLibrary(
    name="members", flags=_NO_CONTRACT,
    #: every kernel the library compiles (tests/test_members_library.py pins this set)
    kernels=("k_members_finish", "k_members_pairs"),
    #: k_members_pairs compiles to 120 VGPRs, no scratch, (4 N_b + 3) x 64 doubles + 64 ints of dynamic LDS (7.9 KB at 3
    #: bands, 67.3 KB at 32) and 4 waves per SIMD: k_cluster_pairs's 78 and on top five more running trapezoids with their
    #: previous products (20 registers), sum_b a_b and sum_b c_b, and two further exponentials in flight.  Its 2 spilled
    #: SGPRs go to VGPR lanes, not to scratch.  On batches the kernel is bound by its instruction stream (DESIGN.md section
    #: 10), which waves beyond the ones that cover the LDS broadcasts do not shorten (a tighter register bound was not tried).
    #: The budget is what it compiles to, the 4-waves-per-SIMD one: 128 VGPRs, and no scratch at all.
    #: k_members_finish (twelve outer trapezoids and their previous terms) is 78 VGPRs at 6 waves
    max_vgpr=128, min_waves=4, extra_headers=("common/last_error.h",))

#: the six libraries the shared builder started with (tests/test_side_libraries_cpu.py pins this tuple to exactly these)
ALL = (CLUSTER, NESTED, SOLVE, DIAG, DERIVED, PREDICT)
#: what __graft_entry__.build() and the command line below build, in order: ALL and the libraries added since ALL was
#: pinned.  A new library goes here; ALL stays what its test says it is
BUILD_ORDER = ALL + (POPULATION,)
#: the libraries added after BUILD_ORDER was pinned in its turn (tests/test_population_library.py); __graft_entry__.build()
#: and the command line below go through BUILD_ORDER + ADDED.  The next library goes here
ADDED = (HIER,)
#: the libraries added after ADDED was pinned in its turn (tests/test_hier_library.py); __graft_entry__.build() and the
#: command line below go through BUILD_ORDER + ADDED + NEWER.  The next library goes here: its test asserts membership,
#: not equality, so this tuple grows
NEWER = (SELECT, REWEIGHT, RELATION, BINNED)
#: the libraries added after NEWER was pinned in its turn (tests/test_side_libraries_cpu.py names its members);
#: __graft_entry__.build() and the command line below go through BUILD_ORDER + ADDED + NEWER + LATEST.  The next library goes
#: here: tests/test_shrink_library.py asserts membership, not equality, so this tuple grows (tests/test_emfit_library.py pins
#: EMFIT as its fourth member, tests/test_members_library.py MEMBERS as its fifth)
LATEST = (SHRINK, DRAW, BINFIT, EMFIT, MEMBERS)


if __name__ == "__main__":
    by_name = {spec.name: spec for spec in BUILD_ORDER + ADDED + NEWER + LATEST}
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(names) != 1 or names[0] not in by_name:
        sys.exit("usage: python -m isochrones_amd.csrc.libraries {%s} [--force] [--verbose]" % ",".join(by_name))
    print(by_name[names[0]].build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
