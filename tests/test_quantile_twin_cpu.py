"""The numpy twin of the chain-quantile kernels (tests/_quantile_twin.py) checked on its own, without a GPU: its answer is
numpy.quantile's, its constants are the sources', and its case set reaches every route of every kernel by the twin's own
replay - the conditions tests/test_gpu_quantile_edges.py relies on when it runs the same cases on the device."""
import collections
import os
import re

import numpy as np
import pytest

from tests import _quantile_twin as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isochrones_amd", "csrc")


def test_mirrored_constants_agree_with_the_sources():
    """A retuned constant fails here; it does not quietly make the routes of the case set vacuous."""
    text = {}
    for name, (rel, pattern, value) in T.SOURCE_CONSTANTS.items():
        if rel not in text:
            with open(os.path.join(CSRC, rel)) as f:
                text[rel] = f.read()
        found = re.findall(pattern, text[rel])
        assert len(found) == 1, "%s: %d matches of %r in %s" % (name, len(found), pattern, rel)
        got = found[0]
        if isinstance(value, int):
            assert int(got) == value, (name, got, value)
        else:
            assert " ".join(got.split()) == value, (name, got, value)
    assert T.QBIG_POOL == T.QSEL_RANKS * T.QBIG_CAP == 2048
    assert (T.QBIG_BINS, T.QBIG_CAP, T.QBIG_NS, T.QSEL_BINS, T.QW_POOL, T.LDS_SORT_MAX) == (4096, 128, 16, 1024, 448, 8192)
    assert (64 * T.QW_IPL, 64 * T.QW_IPL_BIG) == (3328, 6656)


def test_want_is_numpy_quantile_bit_for_bit():
    rng = np.random.default_rng(5)
    levels = np.array((0.0, 1.0) + T.Q7)
    for m in (1, 2, 3, 64, 65, 1110, 8448):
        for x in (rng.standard_normal((3, 2, m)), np.round(rng.standard_normal((3, 2, m)), 1),
                  rng.integers(0, 3, (3, 2, m)).astype(np.float64), np.exp(12 * rng.standard_normal((3, 2, m)))):
            ref = np.moveaxis(np.quantile(x, levels, axis=-1, method="linear"), 0, -1)
            assert np.array_equal(T.want(x, levels), ref), m
    # NaN sorts as +inf: numpy.percentile of the mapped data wherever that is finite, and the same class elsewhere
    x = rng.standard_normal((4, 500))
    x[0, 3] = np.nan
    x[1, :40] = np.nan
    x[2, 7], x[2, 9] = -np.inf, np.nan
    x[3, :] = np.nan
    mapped = np.where(np.isnan(x), np.inf, x)
    with np.errstate(invalid="ignore"):
        ref = np.moveaxis(np.quantile(mapped, levels, axis=-1), 0, -1)       # (percentile without its x100 / 100 round trip)
    got = T.want(x, levels)
    fin = np.isfinite(ref)
    assert fin.sum() >= 16 and np.array_equal(got[fin], ref[fin])
    assert not np.isfinite(got[~fin]).any()
    assert np.isnan(got[3]).all()
    # the lerp next to an infinity, term by term: 2 + inf * 0.2, inf - inf * 0.2, inf - inf; -inf + inf * 0, 1 - inf * 0.4
    assert np.array_equal(T.want([1.0, np.nan, 2.0], [0.6, 0.9, 1.0]), [np.inf, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(T.want([2.0, -np.inf, 1.0], [0.0, 0.3]), [np.nan, -np.inf], equal_nan=True)
    assert np.array_equal(x[0, 3:4], [np.nan], equal_nan=True)                           # the input is not modified


def _case_labels(c):
    """[(pair, kind, [label per target])] of a case by the twin alone"""
    return [(p, kind, labels) for p in c.pairs for kind, labels in T.pair_routes(c.kernels, p.values, c.W, c.q).items()]


def test_every_case_is_on_the_routes_it_is_named_for():
    for c in T.cases():
        assert 2 <= c.S <= 5 and 1 <= c.D <= 4 and 1 <= c.q.size <= 8, c.name
        assert np.all((c.q >= 0) & (c.q <= 1)), c.name
        for p in c.pairs:
            routes = T.pair_routes(c.kernels, p.values, c.W, c.q)
            seen = {lab for labels in routes.values() for lab in labels}
            assert set(p.expect) <= seen, (c.name, p.name, sorted(p.expect), sorted(seen))
            assert not any("unresolved" in lab for lab in seen), (c.name, p.name)
            for level, asked in p.plan.items():
                if c.kernels[0] == "k_chain_quantiles_big":
                    plans = T.big_plan(p.values, c.W, c.q)[2 * level:2 * level + 2]
                elif c.kernels[0] == "k_chain_quantiles_select":
                    plans = [T.select_plan(p.values, c.q)]
                else:
                    plans = [T.wave_plan(p.values, c.q, exact="exact" in c.kernels[0])]
                for plan in plans:
                    for key, value in asked.items():
                        assert value is None or plan[key] == value, (c.name, p.name, level, key, plan)
    # the dispatch the case set relies on
    kernels = {k for c in T.cases() for k in c.kernels}
    assert {"k_chain_quantiles_big", "k_chain_quantiles", "k_chain_quantiles_select", "k_chain_quantiles_wave<52>",
            "k_chain_quantiles_wave<104>", "k_chain_quantiles_exact<12, true>", "k_chain_quantiles_exact<12, false>",
            "k_chain_quantiles_exact<25, false>"} <= kernels
    assert T.case("big_wide_stride").m > 32768 and np.diff(T.sample_positions(33793)).max() == 9 * 256 - 255


def test_wave_cases_do_not_hinge_on_fma_rounding():
    """k_chain_quantiles_exact bins with fma(x, inv, -mn inv): a case whose route the twin decides with unfused arithmetic must
    either bin exactly in both forms (inv zero or a power of two) or sit far from the pool's capacity."""
    n = 0
    for c in T.cases():
        if "exact" not in c.kernels[0]:
            continue
        for p in c.pairs:
            plan = T.wave_plan(p.values, c.q, exact=True)
            if plan["label"] == "flag_overflow":
                assert plan["exact_binning"] or plan["used"] >= 2 * T.QW_POOL, (c.name, p.name, plan)
            elif plan["label"] == "pool":
                assert plan["exact_binning"] or plan["used"] <= T.QW_POOL // 2, (c.name, p.name, plan)
            n += 1
    assert n >= 16
    # the hand-over by the SUM over distinct target bins: more than the pool, no bin more than a list
    for name in ("wave52_routes", "wave104_routes", "exact12_tail_routes", "exact12_routes"):
        c = T.case(name)
        p = [p for p in c.pairs if p.name == "bimodal"][0]
        plan = T.wave_plan(p.values, c.q, exact="exact" in c.kernels[0])
        assert plan["label"] == "flag_overflow" and plan["exact_binning"] and plan["largest"] <= T.QSEL_CAP and plan["bins"] >= 5, plan
        assert T.select_plan(p.values, c.q)["label"] == "lists"


def test_every_route_is_taken_at_least_four_times():
    counts = collections.Counter()
    for c in T.cases():
        for p, kind, labels in _case_labels(c):
            for lab in labels:
                counts["%s %s" % (kind, lab)] += 1
    for key in sorted(counts):
        print("%-44s %5d" % (key, counts[key]))

    def total(kind, pred):
        return sum(n for key, n in counts.items() if key.split()[0] == kind and pred(key.split()[1]))

    for branch in ("neginf", "posinf", "flat", "list", "list_endbin"):
        assert total("big", lambda lab: lab.split(":")[1] == branch) >= 4, branch
    for prefix in ("sampled", "exact_range"):
        assert total("big", lambda lab: lab.split(":")[0] == prefix) >= 4, prefix
    for stem in ("refine_gather", "refine_equal"):
        assert total("big", lambda lab: lab.split(":")[1].split("@")[0] == stem) >= 4, stem
        later = total("big", lambda lab: lab.split(":")[1].split("@")[0] == stem and int(lab.split("@")[1]) >= 1)
        assert later >= 4, (stem, "round 1 or later", later)
    for lab in ("flat", "flag_nonfinite", "flag_overflow", "pool"):
        assert counts["wave " + lab] >= 4, lab
    for lab in ("flat", "sort_nonfinite", "sort_crowded", "lists"):
        assert counts["select " + lab] >= 4, lab
    assert not any("unresolved" in key for key in counts)


def test_extreme_ranges_resolve_in_the_replayed_refinement():
    """The chains whose range, or whose range's reciprocal, overflows: the replay of k_chain_quantiles_big resolves every
    target (on operands scaled by a power of two), within its bound on the rounds; the answers are finite."""
    c = T.case("big_extreme_ranges")
    assert np.isfinite(T.want(c.values, c.q)).all()
    most = 0
    for p in c.pairs:
        plans = T.big_plan(p.values, c.W, c.q)
        assert all("refine" in d["label"] or "list" in d["label"] for d in plans), (p.name, [d["label"] for d in plans])
        most = max([most] + [d.get("rounds", 0) for d in plans])
        print("%-28s %s" % (p.name, sorted({d["label"] for d in plans})))
    # each round divides the interval by about 4 096: 2 098 binades of float64 need at most 175 rounds
    assert 64 < most <= 176 < T.QBIG_ROUNDS, most
    assert np.isfinite(T.want(T.case("wave104_extreme_ranges").values, c.q)).all()
