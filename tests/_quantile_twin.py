"""A plain-numpy twin of the chain-quantile kernels (isochrones_amd/csrc/kernels/k_chain_quantiles.h) and the named case
set the CPU and GPU tests share.  No GPU, no library.

The ANSWER (want): numpy.quantile(method="linear") of the values with NaN mapped to +inf, written out so that the
non-finite cases do not depend on the installed numpy:

    pos = (m - 1) q,  i0 = clamp(floor(pos), 0, m - 1),  i1 = min(i0 + 1, m - 1),  f = pos - i0
    a, b = sorted[i0], sorted[i1];  result = b - (b - a)(1 - f) for f >= 0.5, else a + (b - a) f          (unfused)

The ROUTES: which branch each of the 2 nq target order statistics (i0 and i1 of every level) takes, from a float64
replay of the kernels' decisions.  A pair's values are given in the kernel's own order: value i = (step i // W, walker
i % W).

  routes_big     k_chain_quantiles_big.  "<range>:<branch>" with <range> = sampled | exact_range (the histogram's range
                 from the sample at positions tid + u * sample_stride, or from a pass over every value when the sample has
                 no two distinct finite values) and <branch> =
                   neginf | posinf       the target is one of the -inf / of the +inf and NaN
                   flat                  every finite value equal (exact range only)
                   list | list_endbin    its first-level bin holds at most QBIG_CAP values (list_endbin: bin 0 or the last
                                         bin, and that bin also holds values outside the sampled range)
                   refine_equal@r        round r of the refinement finds every value of the interval equal
                   refine_gather@r       round r's sub-bin fits the pool of QBIG_POOL values
                   unresolved            the rounds ran out (must not happen for any chain)
  routes_wave    k_chain_quantiles_wave<IPL> and, with exact=True, k_chain_quantiles_exact<FULL, TAIL>:
                   flat | flag_nonfinite | flag_overflow | pool       (one decision per pair, repeated for its targets)
  routes_select  k_chain_quantiles_select:
                   flat | sort_nonfinite | sort_crowded | lists       (one decision per pair)

k_chain_quantiles_exact bins with fma(x, inv, -mn inv); numpy cannot fuse.  wave_plan says whether its replay is exact all
the same (inv is zero or a power of two: both products are exact and one rounding is left either way), and the number of
pool slots the pair uses, so that a case can be required to sit well inside its route.

No case holds -0.0 (rounded data has 0.0 added): -0.0 and 0.0 compare equal, so which of the two a sort or a selection puts at a
rank is not defined - by numpy no more than by the kernels - and the bytes of a zero result would be a matter of luck.

The constants are copies; tests/test_quantile_twin_cpu.py reads the sources and asserts that they agree.
"""
import collections
import functools

import numpy as np

# ---- copies of the kernels' constants ------------------------------------------------------------------------------------
BLOCK = 256
QSEL_BINS = 1024
QSEL_CAP = 128
QSEL_RANKS = 16
QBIG_BINS = 4096
QBIG_CAP = 128
QBIG_POOL = QSEL_RANKS * QBIG_CAP        # 2048
QBIG_NS = 16
QBIG_ROUNDS = 256
QW_IPL = 52
QW_IPL_BIG = 104
QW_POOL = 448
LDS_SORT_MAX = 8192                      # the host's `m > 8192` / `A.P < 8192`
EXACT_FULL = (12, 25, 50, 100)

# what the sources must say (name -> (file under isochrones_amd/csrc, regular expression with one group, value))
SOURCE_CONSTANTS = {
    "BLOCK": ("iso_internal.h", r"constexpr\s+int\s+BLOCK\s*=\s*(\d+)\s*;", BLOCK),
    "QSEL_BINS": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QSEL_BINS\s*=\s*(\d+)\s*;", QSEL_BINS),
    "QSEL_CAP": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QSEL_CAP\s*=\s*(\d+)\s*;", QSEL_CAP),
    "QSEL_RANKS": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QSEL_RANKS\s*=\s*(\d+)\s*;", QSEL_RANKS),
    "QBIG_BINS": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QBIG_BINS\s*=\s*(\d+)\s*;", QBIG_BINS),
    "QBIG_CAP": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QBIG_CAP\s*=\s*(\d+)\s*;", QBIG_CAP),
    "QBIG_POOL": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QBIG_POOL\s*=\s*QSEL_RANKS\s*\*\s*QBIG_(CAP)\s*;", "CAP"),
    "QBIG_NS": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QBIG_NS\s*=\s*(\d+)\s*;", QBIG_NS),
    "QBIG_ROUNDS": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QBIG_ROUNDS\s*=\s*(\d+)\s*;", QBIG_ROUNDS),
    "QW_IPL": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QW_IPL\s*=\s*(\d+)\s*;", QW_IPL),
    "QW_IPL_BIG": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QW_IPL_BIG\s*=\s*(\d+)\s*;", QW_IPL_BIG),
    "QW_POOL": ("kernels/k_chain_quantiles.h", r"constexpr\s+int\s+QW_POOL\s*=\s*(\d+)\s*;", QW_POOL),
    "big threshold": ("iso_hip.hip", r"if\s*\(m\s*>\s*(\d+)\)\s*\{\s*\n\s*// longer than the LDS forms hold", LDS_SORT_MAX),
    "sort size": ("iso_hip.hip", r"while\s*\(A\.P\s*<\s*m\s*&&\s*A\.P\s*<\s*(\d+)\)", LDS_SORT_MAX),
    "wave threshold": ("iso_hip.hip", r"else if\s*\(m\s*<=\s*(64)\s*\*\s*QW_IPL_BIG\b", 64),
    "wave<52> threshold": ("iso_hip.hip", r"else if\s*\(m\s*<=\s*(64)\s*\*\s*QW_IPL\)", 64),
    "exact sizes": ("iso_hip.hip", r"((?:ISO_QEXACT\(\d+\)\s*)+)\n\s*default:", " ".join("ISO_QEXACT(%d)" % f for f in EXACT_FULL)),
    "sample stride": ("kernels/k_chain_quantiles.h", r"sample_stride\s*=\s*max\((\d+),\s*\(n_chunks \+ QBIG_NS - 1\) / QBIG_NS\)\s*\*\s*BLOCK", 8),
}


# ---- the answer ----------------------------------------------------------------------------------------------------------
def positions(m, q):
    """(i0, i1, f) of quantile_position for every level of q."""
    q = np.asarray(q, dtype=np.float64)
    pos = np.float64(m - 1) * q
    i0 = np.clip(np.floor(pos), 0, m - 1).astype(np.int64)
    i1 = np.minimum(i0 + 1, m - 1)
    return i0, i1, pos - i0.astype(np.float64)


def target_ranks(m, q):
    """The 2 nq target order statistics in the kernels' order: i0 of level 0, i1 of level 0, i0 of level 1, ..."""
    i0, i1, _ = positions(m, q)
    return np.stack([i0, i1], axis=1).ravel()


def want(values, q):
    """The quantiles q of values[..., m] along the last axis -> [..., nq].  NaN sorts last, as +inf."""
    v = np.array(values, dtype=np.float64)
    v[np.isnan(v)] = np.inf
    v.sort(axis=-1)
    i0, i1, f = positions(v.shape[-1], q)
    a, b = v[..., i0], v[..., i1]
    with np.errstate(invalid="ignore", over="ignore"):
        diff = b - a
        return np.where(f >= 0.5, b - diff * (1 - f), a + diff * f)


# ---- the routes ----------------------------------------------------------------------------------------------------------
def _pair(values):
    v = np.array(values, dtype=np.float64).ravel()
    v[np.isnan(v)] = np.inf
    return v


def _cvt(t):
    """double -> int as the hardware converts: NaN gives 0, the rest saturates."""
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _find_bin(prefix, r):
    """last bin whose exclusive prefix is <= r"""
    return int(np.searchsorted(prefix, r, side="right") - 1)


def _prefix(b, bins):
    h = np.bincount(b, minlength=bins)
    return h, np.concatenate([[0], np.cumsum(h)[:-1]])


def sample_positions(m):
    n_chunks = (m + BLOCK - 1) // BLOCK
    stride = max(8, (n_chunks + QBIG_NS - 1) // QBIG_NS) * BLOCK
    idx = (np.arange(BLOCK)[:, None] + np.arange(QBIG_NS)[None, :] * stride).ravel()
    return np.sort(idx[idx < m])


def big_plan(values, W, q):
    """One dict per target of k_chain_quantiles_big: label, cnt (values in the first-level bin), rounds (refinement rounds
    entered), last (values in the last sub-bin looked at)."""
    v = _pair(values)
    m = v.size
    assert m % W == 0 and m > LDS_SORT_MAX
    sv = v[sample_positions(m)]
    sv = sv[np.isfinite(sv)]
    mn, mx = (sv.min(), sv.max()) if sv.size else (np.inf, -np.inf)
    exact_range = not (mx > mn)
    fin = v[np.isfinite(v)]
    if exact_range:
        mn, mx = (fin.min(), fin.max()) if fin.size else (np.inf, -np.inf)
    binned = bool(mx > mn)
    n_neg, mfin = int((v == -np.inf).sum()), fin.size
    tag = "exact_range:" if exact_range else "sampled:"
    with np.errstate(all="ignore"):
        if binned:
            inv = QBIG_BINS / (mx - mn)
            if not np.isfinite(mx - mn):
                inv = QBIG_BINS / (mx * 0.5 - mn * 0.5) * 0.5
            inv = min(inv, np.finfo(np.float64).max)
            b = np.fmin(np.fmax((fin - mn) * inv, 0.0), QBIG_BINS - 1.0).astype(np.int64)
            h, pre = _prefix(b, QBIG_BINS)
    out = []
    for r in target_ranks(m, q):
        if r < n_neg:
            out.append(dict(label=tag + "neginf"))
        elif r >= n_neg + mfin:
            out.append(dict(label=tag + "posinf"))
        elif not binned:
            out.append(dict(label=tag + "flat"))
        else:
            rank = int(r) - n_neg
            bb = _find_bin(pre, rank)
            cnt, rank = int(h[bb]), rank - int(pre[bb])
            if cnt <= QBIG_CAP:
                vals = fin[b == bb]
                outside = bb in (0, QBIG_BINS - 1) and bool(((vals < mn) | (vals > mx)).any())
                out.append(dict(label=tag + ("list_endbin" if outside else "list"), cnt=cnt))
            else:
                d = _refine(fin, fin[b == bb], rank)
                d.update(label=tag + d["label"], cnt=cnt)
                out.append(d)
    return out


def _refine(fin, vals, rank):
    lo, hi = vals.min(), vals.max()
    last = vals.size
    for rnd in range(QBIG_ROUNDS):
        if not hi > lo:
            return dict(label="refine_equal@%d" % rnd, rounds=rnd, last=last)
        sel = fin[(fin >= lo) & (fin <= hi)]
        with np.errstate(all="ignore"):
            width = hi - lo
            inv2 = QBIG_BINS / width
            if np.isfinite(width) and np.isfinite(inv2):
                b2 = np.minimum(QBIG_BINS - 1, _cvt((sel - lo) * inv2))
            else:        # the range or its reciprocal overflows: the same binning on operands scaled by a power of two
                sc = 2.0 ** 600 if np.isfinite(width) else 0.25
                los = lo * sc
                inv2 = QBIG_BINS / (hi * sc - los)
                b2 = np.fmin(np.fmax((sel * sc - los) * inv2, 0.0), QBIG_BINS - 1.0).astype(np.int64)
        h2, p2 = _prefix(b2, QBIG_BINS)
        k = _find_bin(p2, rank)
        last = int(h2[k])
        if last <= QBIG_POOL:
            return dict(label="refine_gather@%d" % rnd, rounds=rnd + 1, last=last)
        vv = sel[b2 == k]
        lo, hi, rank = vv.min(), vv.max(), rank - int(p2[k])
    return dict(label="unresolved", rounds=QBIG_ROUNDS, last=last)


def routes_big(values, W, q):
    return [d["label"] for d in big_plan(values, W, q)]


def _is_pow2_or_zero(x):
    return x == 0.0 or (np.isfinite(x) and np.frexp(x)[0] == 0.5)


def wave_plan(values, q, exact=False):
    """The decision of a wave kernel for one pair: dict(label, used, exact_binning).  exact=True: the compile-time-shaped
    kernel (a NaN flags the pair; bins from x * inv + (-mn * inv))."""
    raw = np.array(values, dtype=np.float64).ravel()
    v = _pair(raw)
    m = v.size
    mn, mx = v.min(), v.max()
    with np.errstate(all="ignore"):
        inv = QSEL_BINS / (mx - mn)
        degenerate = (not mx > mn) or not np.isfinite(inv) or not np.isfinite(mn) or (exact and bool(np.isnan(raw).any()))
        if degenerate:
            flat = (not mx > mn) and np.isfinite(mn) and np.isfinite(mx) and not (exact and np.isnan(raw).any())
            return dict(label="flat" if flat else "flag_nonfinite", used=0, exact_binning=True)
        if exact:
            b = np.clip(_cvt(v * inv + (-mn * inv)), 0, QSEL_BINS - 1)
        else:
            b = np.minimum(QSEL_BINS - 1, _cvt((v - mn) * inv))
    h, pre = _prefix(b, QSEL_BINS)
    bins = {_find_bin(pre, int(r)) for r in target_ranks(m, q)}
    used = int(sum(h[bb] for bb in bins))
    return dict(label="flag_overflow" if used > QW_POOL else "pool", used=used, exact_binning=(not exact) or _is_pow2_or_zero(inv),
                bins=len(bins), largest=int(max(h[bb] for bb in bins)))


def routes_wave(values, q, exact=False):
    return [wave_plan(values, q, exact)["label"]] * (2 * len(q))


def select_plan(values, q):
    v = _pair(values)
    m = v.size
    mn, mx = v.min(), v.max()
    with np.errstate(all="ignore"):
        inv = QSEL_BINS / (mx - mn)
        degenerate = (not mx > mn) or not np.isfinite(inv) or not np.isfinite(mn)
        if degenerate:
            fallback = mx > mn or not np.isfinite(mn) or not np.isfinite(mx)
            return dict(label="sort_nonfinite" if fallback else "flat", largest=0)
        b = np.minimum(QSEL_BINS - 1, _cvt((v - mn) * inv))
    h, pre = _prefix(b, QSEL_BINS)
    largest = int(max(h[_find_bin(pre, int(r))] for r in target_ranks(m, q)))
    return dict(label="sort_crowded" if largest > QSEL_CAP else "lists", largest=largest)


def routes_select(values, q):
    return [select_plan(values, q)["label"]] * (2 * len(q))


# ---- the host's dispatch -------------------------------------------------------------------------------------------------
def expected_kernels(m, W, mode=None):
    """The kernels iso_chain_quantiles_layout launches for m = nsteps * W values per pair (mode: ISOCHRONES_AMD_QUANTILES)."""
    if m > LDS_SORT_MAX:
        return ["k_chain_quantiles_big"]
    if mode == "sort":
        return ["k_chain_quantiles"]
    if m <= 64 * QW_IPL_BIG and mode != "workgroup":
        if W <= 64 and 64 % W == 0 and mode != "wave" and m // 64 in EXACT_FULL:
            first = "k_chain_quantiles_exact<%d, %s>" % (m // 64, "true" if m % 64 else "false")
        else:
            first = "k_chain_quantiles_wave<%d>" % (QW_IPL if m <= 64 * QW_IPL else QW_IPL_BIG)
        return [first, "k_chain_quantiles_select"]
    return ["k_chain_quantiles_select"]


def pair_routes(kernels, values, W, q):
    """The labels of one pair under the kernels of a case: {"big" | "wave" | "select": [label per target]}; the hand-over
    from a wave kernel to k_chain_quantiles_select is followed."""
    first = kernels[0]
    if first == "k_chain_quantiles_big":
        return {"big": routes_big(values, W, q)}
    if first == "k_chain_quantiles":
        return {}
    if first == "k_chain_quantiles_select":
        return {"select": routes_select(values, q)}
    wave = routes_wave(values, q, exact="exact" in first)
    out = {"wave": wave}
    if wave[0].startswith("flag"):
        out["select"] = routes_select(values, q)
    return out


# ---- the case set --------------------------------------------------------------------------------------------------------
Q7 = (0.5, 0.16, 0.84, 0.0, 1.0, 0.999, 0.3333)                 # the levels of test_chain_quantiles_adversarial_inputs
Q8 = Q7 + (0.05,)
Q_BULK = (0.5, 0.16, 0.84, 0.3333, 0.25, 0.75, 0.05, 0.6)      # both order statistics of every level inside the bulk
TINY = 5e-324

Pair = collections.namedtuple("Pair", "name values expect plan")
# expect: labels that must occur among the pair's targets; plan: {level: {key: value}} asserted on big_plan / wave_plan /
# select_plan of both targets of that level (the capacity edges)


class Case:
    """name, nsteps, W, S, D, q, mode (ISOCHRONES_AMD_QUANTILES or None), kernels (expected trace), pairs (S * D of them, pair
    e * D + d), stream (run on a non-default stream)."""

    def __init__(self, name, nsteps, W, S, D, q, pairs, mode=None, stream=False):
        assert len(pairs) == S * D, (name, len(pairs), S, D)
        self.name, self.nsteps, self.W, self.S, self.D, self.mode, self.stream = name, nsteps, W, S, D, mode, stream
        self.q = np.array(q, dtype=np.float64)
        self.m = nsteps * W
        self.pairs = pairs
        self.kernels = expected_kernels(self.m, W, mode)
        for p in pairs:
            assert p.values.shape == (self.m,), (name, p.name, p.values.shape)

    @property
    def values(self):
        """[S, D, m], value i of a pair = (step i // W, walker i % W)"""
        return np.stack([p.values for p in self.pairs]).reshape(self.S, self.D, self.m)

    def chain(self, param_major):
        """the chain as stored: row-major [nsteps, S * W, D] or parameter-major [nsteps, D, S * W]"""
        x = self.values.reshape(self.S, self.D, self.nsteps, self.W)
        x = x.transpose(2, 1, 0, 3) if param_major else x.transpose(2, 0, 3, 1)
        return np.ascontiguousarray(x).reshape((self.nsteps, self.D, self.S * self.W) if param_major
                                               else (self.nsteps, self.S * self.W, self.D))

    def with_mode(self, mode):
        return Case("%s-%s" % (self.name, mode), self.nsteps, self.W, self.S, self.D, self.q,
                    [Pair(p.name, p.values, (), {}) for p in self.pairs], mode=mode)


def _shuffled(rng, *parts):
    x = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts])
    rng.shuffle(x)
    return x


def _level_at(m, rank):
    """a level whose two order statistics are rank and rank + 1"""
    return (rank + 0.5) / (m - 1)


def _sampled_mask(m):
    s = np.zeros(m, dtype=bool)
    s[sample_positions(m)] = True
    return s


def _big_route_pairs(rng, m):
    P = []
    P.append(Pair("smooth", rng.standard_normal(m), {"sampled:list", "sampled:list_endbin"}, {}))
    P.append(Pair("cluster", _shuffled(rng, 1 + rng.uniform(0, 1e-9, 5000), 1e3 * rng.standard_normal(m - 5000)),
                  {"sampled:refine_gather@1"}, {}))
    P.append(Pair("exp12", np.exp(12 * rng.standard_normal(m)), {"sampled:refine_gather@3", "sampled:refine_gather@4"}, {}))
    P.append(Pair("exp3", np.exp(3 * rng.standard_normal(m)), {"sampled:refine_gather@0"}, {}))
    P.append(Pair("three_valued", rng.integers(0, 3, m).astype(np.float64), {"sampled:refine_equal@0"}, {}))
    P.append(Pair("rounded", np.round(rng.standard_normal(m), 1) + 0.0, {"sampled:refine_equal@0"}, {}))
    x = rng.standard_normal(m)
    x[:100], x[100:300], x[300:400] = -np.inf, np.nan, np.inf
    rng.shuffle(x)
    P.append(Pair("infs_nans", x, {"sampled:neginf", "sampled:posinf", "sampled:list"}, {}))
    s = _sampled_mask(m)
    x = 5 * rng.standard_normal(m)
    x[s] = 0.25
    P.append(Pair("sample_constant", x, {"exact_range:list", "exact_range:refine_gather@0"}, {}))
    x = 5 * rng.standard_normal(m)
    x[s] = rng.uniform(0, 1e-3, int(s.sum()))
    P.append(Pair("sample_narrow", x, {"sampled:refine_gather@0"}, {}))
    x = np.full(m, np.inf)
    x[7] = np.nan
    P.append(Pair("all_inf_one_nan", x, {"exact_range:posinf"}, {}))
    x = np.full(m, 2.5)
    x[300] = np.nan
    P.append(Pair("constant_one_nan", x, {"exact_range:flat", "exact_range:posinf"}, {}))
    # 3 000 copies of 1.0 next to 3 000 values within 1e-9 above it: the rounds narrow down to the copies alone
    P.append(Pair("ties_in_cluster", _shuffled(rng, np.full(3000, 1.0), 1 + rng.uniform(0, 1e-9, 3000),
                                               1e3 * rng.standard_normal(m - 6000)), {"sampled:refine_equal@3"}, {}))
    return P


def _extreme_pairs(rng, m, big):
    """(pairs, q): chains whose range or whose range's reciprocal overflows, and their neighbours; every level in the bulk"""
    P = []
    spots = ((0, 1, "sampled"), (m - 3000, m - 2999, "unsampled")) if big else ((0, 1, "first"),)
    for huge, tag in ((1.7e308, "1p7e308"), (8e307, "8e307")):
        for i, j, where in spots:
            x = rng.standard_normal(m)
            x[i], x[j] = huge, -huge
            P.append(Pair("outliers_%s_%s" % (tag, where), x, (), {}))
    P.append(Pair("subnormal_ladder", rng.integers(0, 2000, m) * TINY, (), {}))
    P.append(Pair("zero_against_tiny", _shuffled(rng, np.zeros(m // 2), np.full(m - m // 2, TINY)), (), {}))
    P.append(Pair("one_ulp_apart", _shuffled(rng, np.full(m // 3, 1.0), np.full(m // 3, np.nextafter(1.0, 2.0)),
                                             1e3 * rng.standard_normal(m - 2 * (m // 3))), (), {}))
    # log-uniform over 2 000 binades: every refinement round keeps most of its values in its first sub-bin
    P.append(Pair("two_thousand_binades", 2.0 ** (-rng.uniform(0, 2000, m)), (), {}))
    if big:
        # the SAMPLE is huge and narrow, the bulk far below it: the first bin spans -1.7e308 .. 1.6e308 and is refined
        x = rng.standard_normal(m)
        s = _sampled_mask(m)
        x[s] = rng.uniform(1.6e308, 1.7e308, int(s.sum()))
        x[np.flatnonzero(~s)[17]] = -1.7e308
        P.append(Pair("refined_range_overflows", x, (), {}))
    return P


def _bimodal(rng, m, nq=8):
    """(values, levels): values 0 .. 1024 with the exact range [0, 1024], so a value's bin of 1 024 is its integer part;
    nb bins hold 120 values each (fractions well inside), the rest is spread thinly.  The levels put targets into every one of
    the heavy bins: together they overflow the wave pool, none overflows a list of the workgroup kernel."""
    nb = min(8, (m - 100) // 120)
    heavy = np.arange(500, 500 + nb)
    n_rest = m - 120 * nb - 2
    n_low = n_rest // 2
    low = rng.integers(1, 500, n_low) + rng.uniform(0.1, 0.9, n_low)
    high = rng.integers(500 + nb, 1023, n_rest - n_low) + rng.uniform(0.1, 0.9, n_rest - n_low)
    dense = (heavy[:, None] + rng.uniform(0.1, 0.9, (nb, 120))).ravel()
    x = _shuffled(rng, [0.0, 1024.0], low, high, dense)
    first = 1 + n_low                                    # rank of the smallest value of the first heavy bin
    q = [_level_at(m, first + 120 * (k % nb) + 60) for k in range(nq)]
    for k in range(nb, nq):                              # the levels left over: into the thin parts
        q[k] = (0.02, 0.97, 0.04)[k - nb]
    return x, q


def _wave_route_pairs(rng, m, exact):
    """8 pairs, one per route of a wave kernel and of the workgroup kernel it hands over to, and the levels (nq = 8)"""
    bim, q = _bimodal(rng, m)
    smooth = rng.standard_normal(m)
    P = [Pair("smooth", smooth, {"pool"}, {}), Pair("constant", np.full(m, 3.25), {"flat"}, {})]
    x = np.full(m, 3.25)
    x[m // 3] = np.nan
    P.append(Pair("constant_one_nan", x, {"flag_nonfinite" if exact else "flag_overflow", "sort_crowded"}, {}))
    x = rng.standard_normal(m)
    x[m // 2] = -np.inf
    P.append(Pair("one_neginf", x, {"flag_nonfinite", "sort_nonfinite"}, {}))
    x = rng.standard_normal(m)
    x[m - 2] = np.nan
    P.append(Pair("one_nan", x, {"flag_nonfinite" if exact else "flag_overflow", "sort_crowded"}, {}))
    P.append(Pair("three_valued", rng.integers(0, 3, m).astype(np.float64), {"flag_overflow", "sort_crowded"}, {}))
    P.append(Pair("bimodal", bim, {"flag_overflow", "lists"}, {}))
    x = rng.standard_normal(m)
    x[5] = np.inf
    P.append(Pair("one_posinf", x, {"flag_overflow", "sort_crowded"}, {}))
    return P, q


def _mixed_pairs(rng, m, n):
    """n pairs of m values for the shape cases: the kinds of data in turn"""
    P = []
    for p in range(n):
        kind = p % 7
        x = rng.standard_normal(m)
        if kind == 1:
            x = np.round(x, 2) + 0.0
        elif kind == 2:
            x[rng.integers(0, m)] = np.nan
        elif kind == 3:
            x[:] = -1.5
        elif kind == 4:
            x[rng.integers(0, m)] = -np.inf
        elif kind == 5:
            x = rng.integers(0, 3, m).astype(np.float64)
        elif kind == 6:
            x[rng.integers(0, m)] = np.inf
        P.append(Pair("mixed%d" % kind, x, (), {}))
    return P


def _one_posinf(rng, m):
    x = rng.standard_normal(m)
    x[m // 2] = np.inf
    return x


def _big_edge_pairs(rng, m):
    """(pairs, q).  Pairs 0 / 1: the sampled range is exactly [0, 4096], a value's first-level bin is its integer part, bin 2000
    holds exactly 128 / 129 values and level 0 / 1 lies in it.  Pairs 2 / 3: inside a spread of width 1e3, a cluster
    [0.25, 0.25 + 2^-30] of more than 2 048 values whose round-1 sub-bins are exactly 2^-42 wide; one of them holds exactly
    2 048 / 2 049 distinct values and level 2 / 3 lies in it."""
    P, q = [], []
    for n_in in (QBIG_CAP, QBIG_CAP + 1):
        n_rest = m - n_in - 2
        n_low = n_rest // 2
        low = rng.integers(1, 2000, n_low) + rng.uniform(0.1, 0.9, n_low)
        high = rng.integers(2001, 4095, n_rest - n_low) + rng.uniform(0.1, 0.9, n_rest - n_low)
        x = _shuffled(rng, low, high, 2000 + rng.uniform(0.1, 0.9, n_in))
        x = np.concatenate([[0.0, 4096.0], x])                          # positions 0 and 1 are sampled
        q.append(_level_at(m, 1 + n_low + n_in // 2))
        label = "sampled:list" if n_in <= QBIG_CAP else "sampled:refine_gather@0"
        P.append(Pair("first_level_bin_of_%d" % n_in, x, {label}, {len(q) - 1: dict(label=label, cnt=n_in)}))
    for n_in in (QBIG_POOL, QBIG_POOL + 1):
        n_cluster_rest = 1500
        n_out = m - n_in - n_cluster_rest - 2
        out = rng.uniform(-500.0, 500.0, n_out)
        # the rest of the cluster: multiples of 2^-54 below 2^-32 and above 2^-31 + 2^-40, off the sub-bin of the n_in values
        off = np.where(rng.random(n_cluster_rest) < 0.4, rng.integers(1, 2 ** 22, n_cluster_rest),
                       rng.integers(2 ** 23 + 2 ** 14, 2 ** 24, n_cluster_rest)) * 2.0 ** -54
        inside = 2.0 ** -31 + np.arange(n_in) * 2.0 ** -54
        cluster = 0.25 + np.concatenate([[0.0, 2.0 ** -30], off, inside])
        x = _shuffled(rng, out, cluster)
        n_below = int((out < 0.25).sum()) + 1 + int((off < 2.0 ** -31).sum())
        q.append(_level_at(m, n_below + n_in // 2))
        label = "sampled:refine_gather@%d" % (1 if n_in <= QBIG_POOL else 2)
        P.append(Pair("round1_sub_bin_of_%d" % n_in, x, {label}, {len(q) - 1: dict(label=label, last=n_in if n_in <= QBIG_POOL else None)}))
    return P, q


@functools.lru_cache(maxsize=None)
def cases():
    """The named cases, built once (seeded).  Both test files use them and leave them unchanged."""
    rng = np.random.default_rng(20240611)
    out = []
    # ---- k_chain_quantiles_big: every route, the capacity edges, the extreme ranges, the shapes ----
    out.append(Case("big_routes", 132, 64, 4, 3, Q8, _big_route_pairs(rng, 8448)))
    P, q = _big_edge_pairs(rng, 8448)
    out.append(Case("big_capacity_edges", 132, 64, 2, 2, q, P))
    out.append(Case("big_extreme_ranges", 132, 64, 3, 3, Q_BULK, _extreme_pairs(rng, 8448, True)))
    m = 33793                                        # 133 chunks: the sample stride is 9 chunks, not 8
    s = _sampled_mask(m)
    x = 5 * rng.standard_normal(m)
    x[s] = 0.25
    y = rng.standard_normal(m)
    y[:100], y[100:300], y[300:400] = -np.inf, np.nan, np.inf
    rng.shuffle(y)
    out.append(Case("big_wide_stride", 719, 47, 2, 2, Q7,
                    [Pair("smooth", rng.standard_normal(m), {"sampled:list"}, {}),
                     Pair("exp3", np.exp(3 * rng.standard_normal(m)), {"sampled:refine_gather@0"}, {}),
                     Pair("sample_constant", x, {"exact_range:list", "exact_range:refine_equal@1"}, {}),      # 4 096 copies: over the pool
                     Pair("infs_nans", y, {"sampled:neginf", "sampled:posinf"}, {})]))
    out.append(Case("big_W8193_one_step", 1, 8193, 2, 1, Q7, _mixed_pairs(rng, 8193, 2)))
    out.append(Case("big_W7", 1207, 7, 3, 1, Q7, _mixed_pairs(rng, 8449, 3)))
    out.append(Case("big_W300", 28, 300, 2, 3, (0.5,), _mixed_pairs(rng, 8400, 6)))
    # ---- the wave kernels and their hand-over: every route, in auto mode and through the workgroup kernel / the sort ----
    for name, nsteps, W in (("wave52", 37, 30), ("wave104", 170, 30), ("exact12_tail", 25, 32), ("exact12", 24, 32)):
        P, q = _wave_route_pairs(rng, nsteps * W, "exact" in name)
        c = Case(name + "_routes", nsteps, W, 4, 2, q, P)
        out += [c, c.with_mode("workgroup"), c.with_mode("sort")]
    out.append(Case("wave104_extreme_ranges", 170, 30, 3, 2, Q_BULK, _extreme_pairs(rng, 5100, False)))
    out.append(out[-1].with_mode("workgroup"))
    # ---- capacity edges: one +inf makes the bin scale 0, every value sits in bin 0 ----
    for m, nsteps, W, mode, label in ((448, 14, 32, None, "pool"), (449, 1, 449, None, "flag_overflow"),
                                      (128, 4, 32, "workgroup", "lists"), (129, 3, 43, "workgroup", "sort_crowded")):
        key = "largest" if mode else "used"
        out.append(Case("edge_%s_%d" % (mode or "pool", m), nsteps, W, 3, 1, Q7,
                        [Pair("one_posinf", _one_posinf(rng, m), {label} | ({"sort_crowded"} if label == "flag_overflow" else set()),
                              {0: {"label": label, key: m}}) for _ in range(3)], mode=mode))
    # ---- shapes ----
    edge_q = (0.0, 1.0, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0), 0.5, 0.25, 0.75, 0.125)
    for m in (1, 2, 63, 64, 65):
        out.append(Case("tiny_m%d_one_step" % m, 1, m, 5, 3, edge_q, _mixed_pairs(rng, m, 15)))
    out.append(Case("tiny_m64_W1", 64, 1, 3, 2, Q7, _mixed_pairs(rng, 64, 6)))
    out.append(Case("nq1", 37, 30, 3, 3, (0.3333,), _mixed_pairs(rng, 1110, 9)))
    out.append(Case("integer_positions", 37, 30, 5, 1, (0.0, 1.0, 100 / 1109, 0.5, 1108 / 1109, 554 / 1109), _mixed_pairs(rng, 1110, 5)))
    out.append(Case("W300_nsteps10", 10, 300, 3, 3, Q8, _mixed_pairs(rng, 3000, 9)))
    out.append(Case("W300_nsteps20", 20, 300, 5, 1, Q8, _mixed_pairs(rng, 6000, 5)))
    out.append(Case("W100_nsteps60", 60, 100, 2, 3, Q7, _mixed_pairs(rng, 6000, 6)))
    out.append(Case("W300_one_step", 1, 300, 5, 2, Q7, _mixed_pairs(rng, 300, 10)))
    out.append(Case("exact25_other_stream", 50, 32, 3, 3, Q8, _mixed_pairs(rng, 1600, 9), stream=True))
    out.append(Case("big_other_stream", 132, 64, 2, 1, Q7, _mixed_pairs(rng, 8448, 2), stream=True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        for p in c.pairs:
            p.values.setflags(write=False)
    return tuple(out)


def case(name):
    return {c.name: c for c in cases()}[name]
