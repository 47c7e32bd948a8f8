"""The cases the binned-population family (libiso_binned.so, libiso_shrink.so, libiso_binfit.so, libiso_emfit.so) is tested
on where the log cell heights of a row, or the start masses of a fit, span hundreds of nats: per-star tables with stars that
have weight only in the cells a row pushes down, rows with those cells at -G and -G / 2 for gaps G on both sides of every
float64 landmark, EM starts with a cell mass down to the smallest subnormal, and the comparison with the long-double twins.
Plain numpy: nothing here touches a GPU or loads a library.

Landmarks, for a table entry of order 1 under a row whose top is 0: at G = 277.3 - ln A the star's s1 = exp(-G) A crosses
ISO_BINNED_RESCUE_BELOW = 2^-400 (THRESHOLD below; :func:`threshold_gaps` gives the two sides for a table's own entry), at
372.2 u * u reaches 0, at 708.4 u goes subnormal, at 745.1 u reaches 0.

Limits (tests/_hier_twin.py's rule).  With span[h, s] = hmx[h] - max{lnh[h, b] : A[b, s] > 0}, the argument of the one
exp a height goes through carries span * 2^-53, so |d ell| <= 1e-11 * max(1, span / 100); ess, N, C and g are held to their
modules' limits (1e-10 relative, 1e-11 max(1, n_live), 1e-11 absolute) times the same factor.  Zeros, -inf, NaN, n_live and
the statuses are compared exactly, and nothing is left out: the twins are finite wherever a star has weight under a row."""
import math

import numpy as np

from tests import _binfit_twin as ft, _binned_twin as bt, _emfit_twin as et

LD = np.longdouble
LOW, MID = 0, 2                                 # the cells a row pushes down: to -G and to -G / 2
THRESHOLD = 2.0 ** -400                         # ISO_BINNED_RESCUE_BELOW
GAPS = (0.0, 100.0, 270.0, 285.0, 360.0, 372.0, 373.0, 500.0, 708.0, 709.0, 740.0, 745.0, 746.0, 760.0, 1500.0)
TOP = 0.3                                       # the largest height of a gap row's other cells
#: star types: weight in every cell; only in LOW; only in LOW and MID; all-zero (mx = -inf); masked
EVERY, ONE, TWO, DEAD, MASKED = "every", "one", "two", "dead", "masked"


def kinds_of(S):
    """The type of each star: S = 6 is the issue's probe (star 4 in LOW only, star 5 in LOW and MID only); a longer catalog
    cycles through the types and ends its first block of 256 and starts its second with stars of the pushed-down cells."""
    if S == 6:
        return [EVERY, EVERY, DEAD, MASKED, ONE, TWO]
    cycle = [EVERY, ONE, EVERY, TWO, DEAD, EVERY, MASKED, EVERY]
    kinds = [cycle[s % len(cycle)] for s in range(S)]
    for s, k in ((250, TWO), (251, ONE), (255, ONE), (256, TWO)):
        if s < S:
            kinds[s] = k
    return kinds


def wide_tables(S, B, seed=0):
    """dict of ``A``, ``A2`` [B, S], ``mx`` [S], ``mask`` [S] int32, ``M`` and ``kinds``: every star's table is summed from
    M = 27 + 2 B per-sample weights exp(-e), e ~ Exp(6) cut at 3.4 and one of them 0, so that A2 is consistent with A and
    every positive entry is at least 1e-3.  mx ~ N(0, 3), two stars at +-1e4."""
    assert B > MID and S >= 6
    rng = np.random.default_rng(100 * S + B + seed)
    M = 27 + 2 * B
    kinds = kinds_of(S)
    A, A2 = np.zeros((B, S)), np.zeros((B, S))
    mx = rng.normal(0.0, 3.0, S)
    for s, kind in enumerate(kinds):
        w = np.exp(-np.minimum(rng.exponential(6.0, M), 3.4))
        w[rng.integers(M)] = 1.0
        if kind == DEAD:
            mx[s] = -np.inf
            continue
        if kind == ONE:
            cell = np.full(M, LOW)
        elif kind == TWO:
            cell = np.where(rng.random(M) < 0.5, LOW, MID)
            cell[:2] = LOW, MID
        else:
            cell = rng.integers(0, B, M)
            cell[:B] = np.arange(B)
        for b in range(B):
            A[b, s], A2[b, s] = w[cell == b].sum(), (w[cell == b] ** 2).sum()
    mx[kinds.index(EVERY)] = 1e4
    mx[len(kinds) - 1 - kinds[::-1].index(TWO)] = -1e4
    mask = np.array([0 if k == MASKED else 1 for k in kinds], np.int32)
    return dict(A=np.ascontiguousarray(A), A2=np.ascontiguousarray(A2), mx=mx, mask=mask, M=M, kinds=kinds)


def threshold_gaps(tab):
    """The two gaps either side of the one at which the first LOW-only star's s1 = exp(-G - TOP) A[LOW] crosses THRESHOLD."""
    a = tab["A"][LOW, tab["kinds"].index(ONE)]
    at = math.log(a) - TOP - math.log(THRESHOLD)
    return (at - 0.01, at + 0.01)


def gap_rows(B, gaps=GAPS):
    """``(lnh [H, B], names)``: one row per gap G with LOW at -G, MID at -G / 2 and the other cells at TOP cos(2 pi b / 3)
    (TOP at cell 3, the row's top, and -TOP / 2 next to it); then the G = 500 row shifted by +700 (hmx takes the shift out: it
    changes nothing but ell, by 700), a row with LOW and MID at -inf, and the same row with NaN in their place."""
    assert B > 3
    base = TOP * np.cos(np.arange(B) * (2.0 * np.pi / 3.0))
    base[3] = TOP
    rows, names = [], []
    for G in gaps:
        r = base.copy()
        r[LOW], r[MID] = -G, -0.5 * G
        rows.append(r)
        names.append("G=%g" % G)
    r = base + 700.0
    r[LOW], r[MID] = 200.0, 450.0
    rows.append(r)
    names.append("G=500+700")
    for fill, name in ((-np.inf, "-inf"), (np.nan, "nan")):
        r = base.copy()
        r[LOW] = r[MID] = fill
        rows.append(r)
        names.append(name)
    return np.ascontiguousarray(rows), names


def case(S, B, seed=0):
    """The tables, and the rows on GAPS and on both sides of the tables' own threshold gap: ``(tab, lnh, names)``."""
    tab = wide_tables(S, B, seed)
    lnh, names = gap_rows(B, tuple(sorted(GAPS + threshold_gaps(tab))))
    return tab, lnh, names


def straddles(tab, lnh):
    """Whether the float64 s1 of the first LOW-only star lies on both sides of THRESHOLD among the finite rows."""
    a = tab["A"][LOW, tab["kinds"].index(ONE)]
    with np.errstate(all="ignore"):
        hmx = np.nanmax(lnh, axis=1)
        s1 = np.exp(lnh[:, LOW] - hmx) * a
    s1 = s1[np.isfinite(lnh[:, LOW])]
    return bool(((s1 >= THRESHOLD) & (s1 < THRESHOLD * 1.1)).any() and ((s1 < THRESHOLD) & (s1 > THRESHOLD / 1.1)).any())


# -- the limits -------------------------------------------------------------------------------------------------------
def factor(A, lnh):
    """max(1, span / 100) [H, S]; 1 where the star has no weight under the row."""
    lnh = np.where(np.isnan(lnh), -np.inf, np.asarray(lnh, np.float64))
    H, S = lnh.shape[0], A.shape[1]
    out = np.ones((H, S))
    for s in range(S):
        on = A[:, s] > 0
        if on.any():
            with np.errstate(invalid="ignore"):
                span = lnh.max(axis=1) - lnh[:, on].max(axis=1)
            out[:, s] = np.where(np.isfinite(span), np.maximum(1.0, span / 100.0), 1.0)
    return out


def _same_special(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN")
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (what, "inf")
    fin = np.isfinite(want)
    assert np.array_equal(got[fin] == 0, want[fin] == 0), (what, "zeros")
    return fin


def assert_binned(out, tab, lnh, what=""):
    """``ell``, ``ess``, ``L``, ``min_ess`` against tests/_binned_twin.py's lnlike and against each other.  Returns
    ``(worst |d ell| / limit, worst |d ess| / limit)``."""
    want = bt.lnlike(tab, lnh, tab["M"], tab["mask"])
    on = tab["mask"] != 0
    f = factor(tab["A"], lnh)
    worst = []
    for k, lim in (("ell", 1e-11 * f), ("ess", 1e-10 * f * np.abs(want["ess"]))):
        fin = _same_special(out[k], want[k], (what, k))
        r = np.abs(out[k][fin] - want[k][fin]) / np.where(lim[fin] > 0, lim[fin], 1.0)
        worst.append(float(r.max()))
        assert worst[-1] <= 1.0, (what, k, worst[-1])
    assert not np.isnan(out["ess"][:, on]).any(), (what, "ess is NaN for an unmasked star")
    assert np.array_equal(out["min_ess"], out["ess"][:, on].min(axis=1)), (what, "min_ess is not the minimum of ess")
    fin = _same_special(out["L"], want["L"], (what, "L"))
    slack = on.sum() * 1e-11 * f.max(axis=1)
    assert np.all(np.abs(out["L"][fin] - want["L"][fin]) <= slack[fin]), (what, "L")
    mine = np.array([math.fsum(r) if np.isfinite(r).all() else -np.inf for r in out["ell"][:, on]])
    assert np.array_equal(np.isinf(out["L"]), np.isinf(mine)) and np.all(np.abs(out["L"][fin] - mine[fin]) <= slack[fin]), (what, "sum")
    fin = _same_special(out["min_ess"], want["min_ess"], (what, "min_ess"))
    assert np.all(np.abs(out["min_ess"] - want["min_ess"])[fin] <= 1e-10 * f.max(axis=1)[fin] * want["min_ess"][fin]), (what, "min_ess")
    return tuple(worst)


def assert_binfit(out, ell, tab, lnh, pairs=True, what=""):
    """``N``, ``C``, ``n_live`` against tests/_binfit_twin.py's moments with both of its identities, row by row within
    LIMIT max(1, n_live) times the row's largest factor; a star is live exactly where ``ell`` [H, S] is finite."""
    A, mask = tab["A"], tab["mask"]
    want = ft.moments(A, lnh, mask)
    assert np.array_equal(out["n_live"], want["n_live"]), (what, out["n_live"], want["n_live"])
    assert np.array_equal(out["n_live"], np.isfinite(ell).sum(axis=1)), (what, "live and finite ell")
    f = factor(A, lnh)[:, mask != 0].max(axis=1)
    worst = 0.0
    for h in range(lnh.shape[0]):
        n, lim = want["n_live"][h:h + 1], ft.LIMIT * f[h]
        w = [ft.close(out["N"][h:h + 1], want["N"][h:h + 1], n, lim),
             ft.close(out["N"][h:h + 1].sum(axis=1), n.astype(LD), n, lim)]
        assert np.array_equal(out["N"][h] == 0, np.asarray(want["N"][h] == 0)), (what, h, "zeros of N")
        if pairs:
            w += [ft.close(out["C"][h:h + 1], want["C"][h:h + 1], n, lim),
                  ft.close(out["C"][h:h + 1].sum(axis=2), out["N"][h:h + 1].astype(LD), n, lim)]
            assert np.array_equal(out["C"][h], out["C"][h].T), (what, h)
        worst = max(worst, max(w))
    return worst


# -- EM starts --------------------------------------------------------------------------------------------------------
TINY = (1e-300, 2.3e-308, 1e-310, 4.9e-324, 0.0)    # the start mass of LOW: small, the smallest normal, subnormals, none
WEIGHTS = (1.0, 3.0, 0.5)                           # of every star of a replicate: w / s1 overflows for some and not others


def em_starts(B):
    """g0 [len(TINY), B]: ordinary masses, LOW at each of TINY and MID at 1e-150 (a LOW-and-MID star's responsibilities are a
    ratio of two tiny products).  The rows are not normalised: the library takes them as they are."""
    g = (1.5 + np.cos(np.arange(B))) / (1.5 * B)
    g0 = np.tile(g, (len(TINY), 1))
    g0[:, LOW], g0[:, MID] = TINY, 1e-150
    return np.ascontiguousarray(g0)


def em_case(S, B, seed=0):
    """The arguments of tests/_emfit_twin.py's call and run: a replicate per (start, weight), r = start * 3 + weight."""
    tab = wide_tables(S, B, seed)
    rng = np.random.default_rng(7 * S + B + seed)
    starts = em_starts(B)
    g0 = np.repeat(starts, len(WEIGHTS), axis=0)
    w = np.tile(np.repeat(np.array(WEIGHTS)[:, None], S, axis=1), (len(TINY), 1))
    return dict(A=tab["A"], scale=np.exp(rng.normal(0.0, 0.5, B)), w=np.ascontiguousarray(w), mask=tab["mask"],
                g0=np.ascontiguousarray(g0))


def em_factor(c):
    """max(1, span / 100) [R] of the start: span = ln max_b v_b - ln max{v_b : A[b][s] > 0}, the largest over the stars."""
    out = np.ones(c["g0"].shape[0])
    with np.errstate(divide="ignore"):
        lnv = np.log(c["g0"].astype(LD)) + np.log(c["scale"].astype(LD))
    f = factor(c["A"], np.asarray(lnv, np.float64))
    return np.maximum(out, f[:, c["mask"] != 0].max(axis=1))


def assert_emfit(out, ref, c, what=""):
    """The library's outputs against tests/_emfit_twin.py's run: counts and statuses equal, no NaN mass, the zeros of ``g``
    exactly, ``g`` within LIMIT absolute, ``objective`` within LIMIT max(1, sum w |ln s1|), ``wsum`` within LIMIT max(1, W),
    each times the replicate's factor.  Returns the largest error over its limit."""
    for k in ("n_iter", "status", "n_live"):
        assert np.array_equal(out[k], ref[k]), (what, k, out[k], ref[k])
    assert not np.isnan(out["g"]).any(), (what, "a NaN mass")
    assert not ((out["status"] == et.EMPTY) & (ref["n_live"] > 0)).any(), (what, "EMPTY with live stars")
    assert np.array_equal(out["g"] == 0, np.asarray(ref["g"] == 0)), (what, "zeros of g")
    lim = et.LIMIT * em_factor(c)
    eg = float(np.max(np.abs(out["g"].astype(LD) - ref["g"]).max(axis=1) / lim))
    eq = float(np.max(np.abs(out["objective"].astype(LD) - ref["objective"]) / np.maximum(1, ref["absln"]) / lim))
    ew = float(np.max(np.abs(out["wsum"].astype(LD) - ref["wsum"]) / np.maximum(1, ref["wsum"]) / lim))
    assert max(eg, eq, ew) <= 1.0, (what, eg, eq, ew)
    return max(eg, eq, ew)
