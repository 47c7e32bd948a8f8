"""Cases whose hyper rows differ inside one row tile, for the four libraries on iso_hier_record rows (hier, select,
reweight, relation).  include/isochrones_amd_hier.h allows any record in any row; PopulationModel.pack gives a column one
kind in all its rows, so the random cases of the twins never put two kinds, two parents or two supports into one tile.

No twin of its own: the cases go through the ``fixed_case`` builders of tests/_hier_twin.py, _select_twin.py,
_reweight_twin.py and _relation_twin.py, and the expected values are those twins'.  A pattern is built once per shape
(``functools.lru_cache``) and must not be changed by a test.

Patterns (``pattern``; values in (0.2, 3) unless said otherwise):
  kinds        Q = 4; row h, column q has kind 1 + (h + q) % 8 of _hier_twin.all_kinds(); interim FLAT, LOGNORMAL, GAUSS,
               POWERLAW: eight consecutive rows hold every kind in every column.
  log_late     Q = 2; interim FLAT; rows GAUSS or FLAT, but the last row POWERLAW: ln x is needed in the last tile only
               (ragged for the H used: its padding repeats that row).
  log_interim  Q = 2; interim LOGNORMAL; no row needs ln x.
  log_early    Q = 2; only row 0 needs ln x.
  supports     Q = 2; FLAT and TRUNCGAUSS rows.  Column 0 of star s is a shuffled linspace over [0.6 + 0.2 s, 2.0 + 0.2 s]
               (spacing below 0.05), and row h has a window [lo, hi] at least 0.4 wide on it, so a (row, star) is dead
               exactly if the window misses the star's interval: ``dead`` says so without evaluating anything.  Rows 0, 1, 2
               of every tile but the last: full support, none, partial, for every star; the other rows slide a window of
               0.4 across [0.1, 2.5]; the rows of the last tile have no support.
  links        relation only, Q = 4, see ``links_rows``.
  edges        see ``edges``.
"""
import functools

import numpy as np

from isochrones_amd import (_cabi, _hier_cabi as hc, _relation_cabi as rl, _reweight_cabi as rc, _select_cabi as sc,
                            hierarchical as hi, priors as P)
from tests import _hier_twin as ht, _relation_twin as rt, _reweight_twin as rw, _select_twin as st

T8, T64, CHUNK = hc.ROW_TILE, rc.ROW_TILE, sc.CHUNK
assert sc.ROW_TILE == T8 == rl.ROW_TILE
PM, RM = _cabi.CHAIN_PARAM_MAJOR, _cabi.CHAIN_ROW_MAJOR
PATTERNS = ("kinds", "log_late", "log_interim", "log_early", "supports")
LOG_KINDS = (hc.POWERLAW, hc.LOGNORMAL, hc.CHABRIER)                # needs_log of csrc/common/family_lnf.h

#: the shapes of tests/test_gpu_mixed_rows.py, which tests/test_mixed_rows_cpu.py runs through the host entries first
WT = [(5, 7), (257, 1)]
HS8 = [T8 + 1, 3 * T8 + 5]
HS64 = [T64 + 1, 150]
JS = [37, 257, CHUNK + 1]
#: (pattern, W, T, H, layout) for hier and relation: every pattern at both M and both H, the row-major layout once each
CHAIN_SHAPES = [(name, W, T, H, RM if (i + j + k) % 4 == 0 else PM) for i, name in enumerate(PATTERNS)
                for j, (W, T) in enumerate(WT) for k, H in enumerate(HS8)]
SELECT_SHAPES = [(name, J, H) for name in PATTERNS for J in JS for H in HS8]
REWEIGHT_SHAPES = [(name, W, T, H, RM if (i + j + k) % 4 == 0 else PM) for i, name in enumerate(PATTERNS)
                   for j, (W, T) in enumerate(WT) for k, H in enumerate(HS64)]
#: (H, W, T, layout) of the links pattern: the last row linked (its padding repeats a linked row), the last row unlinked,
#: and three tiles and five rows
LINK_SHAPES = [(2 * T8 + 3, 5, 7, PM), (2 * T8 + 2, 5, 7, RM), (2 * T8 + 3, 257, 1, RM), (2 * T8 + 2, 257, 1, PM),
               (3 * T8 + 5, 5, 7, PM), (3 * T8 + 5, 257, 1, PM)]
#: every kind of _hier_twin.all_kinds() as the interim record and as a row record
EDGE_CASES = [(kind, role) for kind in range(1, 9) for role in ("interim", "row")]


# -- records ----------------------------------------------------------------------------------------------------------
def flat(lo, hi_):
    return hi.prior_record(P.FlatPrior((lo, hi_)))


def gauss(mean, sigma):
    return hi.prior_record(P.GaussianPrior(mean, sigma, bounds=(0.1, 10.0)))


def powerlaw(alpha):
    return hi.prior_record(P.PowerLawPrior(alpha, (0.1, 10.0)))


def lognormal(mu, sigma):
    return hi.prior_record(P.LogNormalPrior(mu, sigma))


def truncgauss(lo, hi_, mean, sigma):
    rec = hi.records(1)
    hi.TruncatedGaussian((lo, hi_)).fill(rec, np.array([[mean, sigma]]))
    return rec


def _plain(h, q):
    """a row record that needs no ln x: GAUSS and FLAT in turn, the parameters moving with the row"""
    if (h + q) % 2 == 0:
        return gauss(0.8 + 0.1 * ((h + q) % 7), 0.4 + 0.05 * (h % 5))
    return flat(0.1, 4.0 + (h + q) % 5)


def log_tiles(interim, rows, tile):
    """[ntiles, Q] bool: does the kernel compute ln x for (tile, column)?  The OR of needs_log over the interim record and
    the tile's rows; the padding of a ragged tile repeats its last row, which is one of them."""
    H, Q = rows.shape
    own = np.isin(interim["kind"], LOG_KINDS)
    return np.array([own | np.isin(rows[h0:h0 + tile]["kind"], LOG_KINDS).any(axis=0) for h0 in range(0, H, tile)])


# -- the patterns -----------------------------------------------------------------------------------------------------
def _window(h, H, tile):
    """the support [lo, hi] of row h on column 0 of the supports pattern"""
    if h >= ((H - 1) // tile) * tile:
        return 4.0, 5.0                                             # the last tile: no support for any star
    j = h % 8
    if j < 3:
        return ((0.5, 2.5), (4.0, 5.0), (1.2, 1.6))[j]              # full, none, partial: the dead row between live ones
    k = (3 * h) % 11
    return 0.1 + 0.2 * k, 0.5 + 0.2 * k


def star_interval(s):
    return 0.6 + 0.2 * s, 2.0 + 0.2 * s


def pattern(name, S, M, H, tile, seed=0):
    """``dict(x [Q, S, M], interim [Q] records, rows [H][Q] records, dead [H, S] or None)``."""
    rng = np.random.default_rng(100 + seed)
    kinds = ht.all_kinds()
    Q = 4 if name == "kinds" else 2
    x = rng.uniform(0.2, 3.0, (Q, S, M))
    dead = None
    if name == "kinds":
        interim = [kinds[hc.FLAT], kinds[hc.LOGNORMAL], kinds[hc.GAUSS], kinds[hc.POWERLAW]]
        rows = [[kinds[1 + (h + q) % 8] for q in range(Q)] for h in range(H)]
    elif name in ("log_late", "log_early", "log_interim"):
        interim = [lognormal(0.0, 0.5), lognormal(0.2, 0.6)] if name == "log_interim" else [flat(0.1, 10.0)] * 2
        rows = [[_plain(h, q) for q in range(Q)] for h in range(H)]
        if name != "log_interim":
            rows[H - 1 if name == "log_late" else 0] = [powerlaw(-2.35), powerlaw(-0.5)]
    elif name == "supports":
        interim = [flat(0.1, 10.0)] * 2
        for s in range(S):
            a, b = star_interval(s)
            x[0, s] = rng.permutation(np.linspace(a, b, M))
        rows, dead = [], np.zeros((H, S), bool)
        for h in range(H):
            lo, hi_ = _window(h, H, tile)
            first = flat(lo, hi_) if (h // 8 + h) % 2 == 0 else truncgauss(lo, hi_, 0.5 * (lo + hi_), 0.5)
            second = truncgauss(0.1, 10.0, 1.0 + 0.1 * (h % 5), 0.7) if h % 2 else flat(0.1, 10.0)
            rows.append([first, second])
            dead[h] = [hi_ < star_interval(s)[0] or lo > star_interval(s)[1] for s in range(S)]
    else:
        raise ValueError(name)
    return dict(x=x, interim=interim, rows=rows, dead=dead)


def support_of_rows(case_x0, rows):
    """[H, n] bool from the inputs alone: is value ``case_x0[i]`` inside the window of row h's column-0 record?"""
    lo, hi_ = rows[:, 0]["lo"][:, None], rows[:, 0]["hi"][:, None]
    return (case_x0[None, :] >= lo) & (case_x0[None, :] <= hi_)


def links_rows(H, link3=True):
    """Q = 4, column 1 the child: rows h % 3 == 0 follow column 0, rows h % 3 == 1 column 2 (the parent above its child),
    rows h % 3 == 2 are unlinked, TRUNCGAUSS and POWERLAW in turn (the power law makes an unlinked row of a linked column
    need ln x).  With ``link3`` column 3 follows column 1 in the odd rows.  Columns 0 and 2 walk through the kinds."""
    kinds = ht.all_kinds()
    rows = []
    for h in range(H):
        if h % 3 == 2:
            child = truncgauss(0.1, 10.0, 1.2 + 0.1 * (h % 4), 0.8) if (h // 3) % 2 == 0 else powerlaw(-1.5 - 0.1 * (h % 4))
        else:
            child = rt.link(0.1, 10.0, 0 if h % 3 == 0 else 2, 1.0 + 0.1 * (h % 5), 0.3 - 0.1 * (h % 4), 0.5 + 0.05 * (h % 3),
                            pivot=1.5)
        if link3 and h % 2 == 1:
            last = rt.link(0.1, 10.0, 1, 1.4 - 0.1 * (h % 5), 0.2 * (h % 3) - 0.2, 0.6, pivot=1.5)
        else:
            last = _plain(h, 3)
        rows.append([kinds[1 + h % 8], child, kinds[1 + (h + 3) % 8], last])
    return rows


def parent_of(rows):
    """[H, Q] int: the parent column of a linked record, -1 for an unlinked one"""
    return np.where(rows["kind"] == rl.LINGAUSS, rows["reserved"], -1)


def edge_values(rec):
    """The sample values at the edges of the record ``rec`` ([1])."""
    lo, hi_ = float(rec["lo"][0]), float(rec["hi"][0])
    v = [lo, hi_, np.nextafter(lo, -np.inf), np.nextafter(hi_, np.inf), 0.0, -0.0, -0.5, np.inf, -np.inf, 5e-324]
    if int(rec["kind"][0]) == hc.CHABRIER:
        brk = float(rec["p"][0, 5])
        v += [brk, np.nextafter(brk, -np.inf), np.nextafter(brk, np.inf)]
    return np.array(v)


#: where the edge values go (M = 257): the first and last lane of a wavefront, the last lane of the workgroup and the lone
#: sample of the second pass first; star s shifts the values by 5 s places, so with three stars every value meets those five
#: in some star (the two stars of a reweight case leave three of CHABRIER's thirteen at the other places)
EDGE_AT = [0, 63, 64, 255, 256, 1, 62, 65, 127, 128, 191, 192, 254]
EDGE_M = 257
WIDE, NARROW, LOW, LOW_REWEIGHT = (-20.0, 20.0), (0.05, 20.0), (-1.0, 0.15), (0.06, 0.15)


def edges(kind, role, H, S=3, seed=0, low=LOW):
    """One column (two for LINGAUSS: the interior parent first) of interior values in (0.2, 3) with ``edge_values`` of the
    record of ``kind`` at ``EDGE_AT``.  role "interim": the record is the interim prior, the even rows FLAT on NARROW (inside
    it: lo, hi and the interior; below it 0, -0, the negative value and the subnormal), the odd rows FLAT on LOW (no interior
    value; lo if it is 0.1).  role "row": the interim prior FLAT on WIDE (only +-inf are bad), the even rows the record, the
    odd rows FLAT on LOW.  ``low``: another window for LOW."""
    rng = np.random.default_rng(200 + 16 * seed + kind)
    if kind == rl.LINGAUSS:
        assert role == "row"
        rec = rt.link(0.1, 10.0, 0, 1.0, 0.3, 0.6, pivot=1.5)
    else:
        rec = ht.all_kinds()[kind]
    vals = edge_values(rec)
    n = len(vals)
    x = rng.uniform(0.2, 3.0, (1, S, EDGE_M))
    for s in range(S):
        for i, v in enumerate(vals):
            x[0, s, EDGE_AT[(i + 5 * s) % n]] = v
    interim = [rec] if role == "interim" else [flat(*WIDE)]
    even = flat(*NARROW) if role == "interim" else rec
    rows = [[even] if h % 2 == 0 else [flat(*low)] for h in range(H)]
    if kind == rl.LINGAUSS:
        x = np.concatenate([rng.uniform(0.2, 3.0, (1, S, EDGE_M)), x])
        interim = [flat(*WIDE)] + interim
        rows = [[gauss(1.0, 0.5) if h % 2 == 0 else flat(0.1, 10.0)] + r for h, r in enumerate(rows)]
    return dict(x=x, interim=interim, rows=rows, dead=None)


#: by hand, for the records with lo = 0.1, hi = 10 (FLAT, POWERLAW, LINGAUSS), per star.  role "interim": lo and hi are
#: inside, their outer neighbours, 0, -0, -0.5, +-inf and the subnormal outside: 8 bad; an odd row (LOW) keeps lo alone, so
#: ess = 1.  role "row": +-inf are bad; an odd row keeps lo, its lower neighbour, 0, -0, -0.5 and the subnormal at one
#: weight, so ess = 6; no row keeps hi's upper neighbour, so with +-inf three samples weigh nothing under all rows.
EDGE_BY_HAND = {"interim": dict(n_bad=8, odd_ess=1.0, zero_weights=8), "row": dict(n_bad=2, odd_ess=6.0, zero_weights=3)}
HAND_KINDS = (hc.FLAT, hc.POWERLAW, rl.LINGAUSS)


def check_edges_by_hand(kind, role, got):
    """``got``: ell, ess [H, S] and n_bad [S] (or the select results as [H, 1] and [1])"""
    if kind not in HAND_KINDS:
        return
    hand = EDGE_BY_HAND[role]
    assert (np.asarray(got["n_bad"]) == hand["n_bad"]).all()
    assert np.isfinite(got["ell"]).all() and (got["ess"][1::2] == hand["odd_ess"]).all()


def check_edge_weights(kind, role, case, got, want):
    bad = np.zeros(want["weights"].shape, bool)
    for s in range(bad.shape[0]):
        l0 = ht.lnf(case["interim"][0], case["x"][0, s])
        bad[s] = np.isnan(case["x"][0, s]) | np.isnan(l0) | np.isneginf(l0)
    assert np.array_equal(bad.sum(axis=1), want["n_bad"]) and (got["weights"][bad] == 0.0).all()
    assert np.array_equal(got["weights"] == 0.0, want["weights"] == 0.0)
    if kind in HAND_KINDS:
        hand = EDGE_BY_HAND[role]
        assert (got["n_bad"] == hand["n_bad"]).all() and ((got["weights"] == 0.0).sum(axis=1) == hand["zero_weights"]).all()


# -- the cases, once per shape ----------------------------------------------------------------------------------------
def _pattern_or_edges(name, S, M, H, tile, seed, low=LOW):
    if isinstance(name, tuple):                                     # ("edges", kind, role)
        assert M == EDGE_M
        return edges(name[1], name[2], H, S, seed, low)
    return pattern(name, S, M, H, tile, seed)


@functools.lru_cache(maxsize=None)
def chain_case(name, W, T, H, layout=PM, seed=0):
    """A tests/_hier_twin.py case (hier, and relation through _relation_twin.call) with ``dead`` [H, S] or None."""
    p = _pattern_or_edges(name, 3, W * T, H, T8, seed)
    case = ht.fixed_case(p["x"], p["interim"], p["rows"], W, T, layout, seed=seed)
    case["dead"] = p["dead"]
    return case


@functools.lru_cache(maxsize=None)
def links_case(H, W, T, layout=PM, link3=True, bad=None, seed=0):
    """The links pattern; ``bad`` = (row, reserved) gives that row's column-1 record an invalid parent."""
    rng = np.random.default_rng(300 + seed)
    kinds = ht.all_kinds()
    x = rng.uniform(0.2, 3.0, (4, 3, W * T))
    interim = [kinds[hc.FLAT], kinds[hc.LOGNORMAL], kinds[hc.GAUSS], kinds[hc.POWERLAW]]
    case = ht.fixed_case(x, interim, links_rows(H, link3), W, T, layout, seed=seed)
    if bad is not None:
        assert case["rows"][bad[0], 1]["kind"] == rl.LINGAUSS
        case["rows"][bad[0], 1]["reserved"] = bad[1]
    return case


@functools.lru_cache(maxsize=None)
def select_case(name, J, H, seed=0):
    """A tests/_select_twin.py case.  supports: the stars of the chain cases become the chunks (``dead`` [H, chunks]); the
    first chunk is star 0's interval; with J = CHUNK + 1 the second chunk is the one injection 2.3, outside it, so a window
    has support in one chunk, in the other, in both or in none (partial support needs two injections: first chunk only)."""
    rng = np.random.default_rng(400 + seed)
    p = _pattern_or_edges(name, 3 if isinstance(name, tuple) else 1, J, H, T8, seed)
    x = p["x"][:, seed % 3 if isinstance(name, tuple) else 0, :].copy()
    lnd = st._lnd(rng, J)
    dead = None
    if isinstance(name, tuple):
        lnd[:] = 0.0                                                # every injection detected: the counts by hand hold
    if name == "supports":
        lnd = np.where(np.isneginf(lnd), np.log(0.5), lnd)          # every injection detectable: ``dead`` is the windows'
        n0 = min(J, CHUNK)
        a, b = star_interval(0)
        x[0, :n0] = rng.permutation(np.linspace(a, b, n0))
        x[0, n0:] = 2.3
        ends = [(a, b)] + ([(2.3, 2.3)] if J > CHUNK else [])
        rows = np.stack([np.concatenate(r) for r in p["rows"]])
        dead = np.array([[r["hi"] < lo or r["lo"] > hi_ for lo, hi_ in ends] for r in rows[:, 0]])
    case = st.fixed_case(x, lnd, p["interim"], p["rows"])
    case["dead"] = dead
    return case


@functools.lru_cache(maxsize=None)
def reweight_case(name, W, T, H, layout=PM, seed=0):
    """A tests/_reweight_twin.py case with S = 2 stars, V = 2 value columns of its own and K = 3 probabilities.

    edges, role "interim": the odd rows are FLAT on LOW_REWEIGHT, which keeps lo = 0.1 and leaves the subnormal out.  Under a
    LOGNORMAL interim prior ln f0(5e-324) = -1.1e6, so a row with support there has r = 1.1e6 on that sample alone,
    ln_norm = ell = r - ln M, and the weight exp(r - ln_norm) carries the rounding of r itself, an ulp of 1.1e6 = 2.3e-10,
    while tests/_reweight_twin.py scales its limit by |r - ln_norm| = ln M (1e-11).  The host entry misses that limit
    17-fold there, by the float64 of r and not by its arithmetic; the hier, select and relation cases keep that sample (their
    limits scale with |r|)."""
    S = 2
    low = LOW_REWEIGHT if isinstance(name, tuple) and name[2] == "interim" else LOW
    p = _pattern_or_edges(name, S, W * T, H, T64, seed, low)
    y = np.random.default_rng(500 + seed).normal(size=(2, S, W * T))
    case = rw.fixed_case(p["x"], y, p["interim"], p["rows"], W, T, rw.PROBS3, layout, seed=seed)
    case["dead"] = p["dead"]
    return case


# -- the largest error over the twins' limits -------------------------------------------------------------------------
def over_limit(got, want, key="ell", scale="rmax"):
    """max |got - want| / limit of tests/_hier_twin.py (key "ell", scale "rmax") or tests/_select_twin.py ("ln_alpha",
    "tmax") over the finite entries."""
    fin = np.isfinite(want[key])
    lim = 1e-11 * np.maximum(1.0, want[scale] / 100.0)
    with np.errstate(invalid="ignore"):
        d = np.abs(got[key] - want[key])
    return float(np.max(d[fin] / lim[fin])) if fin.any() else 0.0


def over_limit_weights(got, want):
    """the same for the weights of tests/_reweight_twin.py"""
    live = ~np.isnan(want["wsum"])
    gu, wu = got["weights"][live], want["weights"][live]
    lim = (1e-11 * np.maximum(1.0, want["dmax"][live] / 100.0))[:, None]
    return float(np.max(np.abs(gu - wu) / (lim * wu + 1e-300)))
