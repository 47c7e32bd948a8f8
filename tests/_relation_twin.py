"""A long-double numpy statement of include/isochrones_amd_relation.h (the linked population likelihood of
libiso_relation.so) on top of tests/_hier_twin.py, the cases its host and device tests share, and the one way they call the
library.

The kinds 1 .. 8 are _hier_twin.lnf.  The linked kind is evaluated in long double with the truncation mass from float64
scipy.special.erfc on the header's flipped form.  That form was measured within 2.5e-13 relative of mpmath at 40 digits
over 20 000 draws with means up to 80 sigma outside the bounds; it is exactly 0 beyond about 38 sigma.  So the limits are
_hier_twin's (|d ell| <= 1e-11 * max(1, max_m |r| / 100), ess within 1e-10 relative, -inf, NaN and n_bad exact), and the
random cases keep every mean within 40 sigma of the bounds (they stay within 13)."""
import numpy as np
from scipy.special import erfc

from isochrones_amd import _cabi, _hier_cabi as hc, _relation_cabi as rl, hierarchical as hi, priors as P, relations
from tests import _hier_twin as tw

LD = tw.LD
ROOT_HALF = 0.7071067811865476


def lingauss(rec, x, xp):
    """ln f(x; rec) of a LINGAUSS record given the parent's values ``xp``, in long double."""
    x, xp = np.asarray(x, np.float64).astype(LD), np.asarray(xp, np.float64).astype(LD)
    p = [LD(v) for v in rec["p"]]
    lo, hi_ = LD(rec["lo"]), LD(rec["hi"])
    with np.errstate(all="ignore"):
        mu = p[0] + p[4] * (xp - p[5])
        z = (x - mu) * p[3]
        a, b = (lo - mu) * p[3], (hi_ - mu) * p[3]
        flip = a > 0
        a, b = np.where(flip, -b, a), np.where(flip, -a, b)
        mass = 0.5 * (erfc((-b * LD(ROOT_HALF)).astype(np.float64)) - erfc((-a * LD(ROOT_HALF)).astype(np.float64)))
        v = (-(z * z) / 2 + p[2]) - np.log(mass.astype(LD))
        v = np.where(mass > 0, v, LD(-np.inf))              # a NaN mass (NaN parent) too
    return np.where((x < lo) | (x > hi_), LD(-np.inf), v)


def term(rec, q, xs):
    """The population term of column ``q`` for the sample values ``xs`` [Q, M]."""
    if int(rec["kind"]) != rl.LINGAUSS:
        return tw.lnf(rec, xs[q])
    p, Q = int(rec["reserved"]), xs.shape[0]
    if not 0 <= p < Q or p == q:
        return np.full(xs.shape[1], LD(np.nan))
    return lingauss(rec, xs[q], xs[p])


def lnlike(x, interim, rows, mask=None):
    """_hier_twin.lnlike with the linked kind among the rows' records."""
    Q, S, M = x.shape
    H = rows.shape[0]
    ell, ess, rmax = np.empty((H, S), LD), np.empty((H, S), LD), np.zeros((H, S))
    n_bad = np.zeros(S, np.int32)
    with np.errstate(all="ignore"):
        for s in range(S):
            if mask is not None and not mask[s]:
                ell[:, s] = ess[:, s] = np.nan
                continue
            l0 = [tw.lnf(interim[q], x[q, s]) for q in range(Q)]
            good = np.ones(M, bool)
            for q in range(Q):
                good &= ~np.isnan(x[q, s]) & ~np.isnan(l0[q]) & (l0[q] != -np.inf)
            n_bad[s] = M - good.sum()
            for h in range(H):
                r = np.zeros(M, LD)
                for q in range(Q):
                    lf = term(rows[h, q], q, x[:, s])
                    lf = np.where(np.isnan(lf), LD(-np.inf), lf)
                    r = lf - l0[q] if q == 0 else r + (lf - l0[q])
                r = r[good]
                fin = r[np.isfinite(r)]
                if fin.size == 0:
                    ell[h, s], ess[h, s] = -np.inf, 0
                    continue
                mx = r.max()
                w = np.exp(r - mx)
                ell[h, s] = mx + np.log(w.sum()) - np.log(LD(M))
                ess[h, s] = w.sum() ** 2 / (w * w).sum()
                rmax[h, s] = float(np.abs(fin).max())
        keep = np.ones(S, bool) if mask is None else np.asarray(mask) != 0
        L = ell[:, keep].sum(axis=1) if keep.any() else np.zeros(H)
        mn = ess[:, keep].min(axis=1) if keep.any() else np.full(H, np.inf)
    return dict(ell=ell.astype(np.float64), ess=ess.astype(np.float64), n_bad=n_bad, L=np.asarray(L, np.float64),
                min_ess=np.asarray(mn, np.float64), rmax=rmax)


def want(case):
    if "want" not in case:
        case["want"] = lnlike(case["x"], case["interim"], case["rows"], case["mask"])
    return case["want"]


assert_matches = tw.assert_matches

# -- cases ------------------------------------------------------------------------------------------------------------
#: per column type of _hier_twin.COLUMN_TYPES: the bounds of a family on it, a pivot, and the largest |x - pivot| it draws
_TYPES = ((0.1, 10.0, 1.0, 8.0), (-4.0, 0.5, -0.1, 3.4), (5.0, 10.15, 9.3, 0.8), (0.0, 1.0, 0.5, 0.5))


def link_records(rng, H, child_type, parent_type, parent):
    """H LINGAUSS records on a column of ``child_type`` that follow column ``parent`` of ``parent_type``: the mean stays
    within a quarter of the span outside the bounds and sigma is at least 0.02 spans, so within 12.5 sigma of them."""
    lo, hi_, _, _ = _TYPES[child_type]
    _, _, pivot, reach = _TYPES[parent_type]
    span = hi_ - lo
    theta = np.column_stack([rng.uniform(lo + 0.25 * span, hi_ - 0.25 * span, H), rng.uniform(-1.0, 1.0, H) * 0.5 * span / reach,
                             rng.uniform(0.02, 0.4, H) * span])
    rec = hi.records(H)
    relations.LinearGaussian("parent", (lo, hi_), (-100.0, 100.0), pivot=pivot).fill(rec, theta)
    rec["reserved"] = parent
    return rec


def linked_case(S, W, T, Q, H, seed, links, layout=_cabi.CHAIN_PARAM_MAJOR, split=True):
    """_hier_twin.random_case with the population records of every child of ``links`` = {child: parent} linked."""
    case = tw.random_case(S, W, T, Q, H, seed, layout=layout, split=split)
    rng = np.random.default_rng(7000 + seed)
    rows = case["rows"].copy()
    for child, parent in links.items():
        rows[:, child] = link_records(rng, H, (child + seed) % 4, (parent + seed) % 4, parent)
    case["rows"] = rows
    return case


PM, RM, TILE = _cabi.CHAIN_PARAM_MAJOR, _cabi.CHAIN_ROW_MAJOR, rl.ROW_TILE
#: test_gpu_hier.py's shapes, each with its links {child: parent}
#          S, W,  T,  Q, H,            layout, links
SHAPES = [(3, 5,  7,  2, 1,            PM, {1: 0}),                  # M = 35, one link across two storages
          (3, 5,  7,  4, 3 * TILE + 5, RM, {1: 0, 3: 1}),            # a chain of links
          (3, 5,  7,  4, TILE + 1,     PM, {0: 2}),                  # the parent's index above its child's
          (3, 64, 1,  4, TILE,         PM, {1: 0, 3: 1}),
          (3, 64, 1,  2, TILE + 1,     RM, {0: 1}),
          (2, 40, 30, 2, TILE + 1,     PM, {1: 0}),                  # M = 1200
          (2, 40, 30, 4, 1,            RM, {0: 2, 3: 0}),
          (2, 40, 30, 4, 3 * TILE + 5, PM, {1: 0, 3: 1})]


def link(lo, hi_, parent, intercept, slope, sigma, pivot=0.0):
    """One LINGAUSS record, shape [1]."""
    rec = hi.records(1)
    relations.LinearGaussian("parent", (lo, hi_), (-1e3, 1e3), pivot=pivot).fill(rec, np.array([[intercept, slope, sigma]]))
    rec["reserved"] = parent
    return rec


def special_cases():
    """name -> case, two columns (0: the parent, 1: the child) unless said otherwise."""
    rng = np.random.default_rng(15)
    W, T, S = 5, 7, 3
    M = W * T
    flat = P.FlatPrior((-4.0, 4.0))
    par = P.GaussianPrior(0.0, 1.0)
    out = {}
    ordinary = [[par, link(-3.0, 3.0, 0, 0.1, 0.5, 0.4)], [par, link(-3.0, 3.0, 0, -0.2, -0.8, 0.7)]]
    x = rng.normal(0.0, 0.5, (2, S, M))
    x[0, 0, 3] = np.nan                                             # the parent alone
    x[0, 2, 7] = x[1, 2, 7] = np.nan                                # both: counted once
    x[1, 2, 9] = np.nan                                             # the child alone
    out["parent_nan"] = tw.fixed_case(x, [flat, flat], ordinary, W, T)
    x = rng.normal(0.0, 0.5, (2, S, M))
    x[1, 1] = rng.uniform(3.1, 3.9, M)                              # star 1: every child outside the family's bounds, inside
    x[1, 0, :5] = -3.5                                              # the interim prior's; star 0: five of them
    out["child_out"] = tw.fixed_case(x, [flat, flat], ordinary, W, T)
    x = rng.normal(0.0, 0.5, (2, S, M))
    # row 0: the mean is 3 + 60 * 0.05 + 0.5 * xp, xp > -4: more than 60 sigma above the bounds for every sample
    out["mean_60_sigma"] = tw.fixed_case(x, [flat, flat], [[par, link(-3.0, 3.0, 0, 8.0, 0.5, 0.05)], ordinary[0]], W, T)
    bad = [link(-3.0, 3.0, 0, 0.1, 0.5, 0.4) for _ in range(3)]
    bad[0]["reserved"], bad[1]["reserved"], bad[2]["reserved"] = 1, 2, -1        # itself, past Q, negative
    out["bad_parent"] = tw.fixed_case(x, [flat, flat], [[par, b] for b in bad] + [ordinary[0]], W, T)
    out["masked"] = tw.fixed_case(x, [flat, flat], ordinary, W, T, mask=[1, 0, 1])
    x = np.empty((2, S, M))
    x[0] = rng.uniform(0.0, 1.0, (S, M))
    for s in range(S):
        x[1, s] = rng.permutation(np.linspace(0.0, 37.4, M))       # r = x^2 / 2 - (x - mu)^2 / 2, mu near 37.4: -699 .. +699
    out["span_700"] = tw.fixed_case(x, [P.FlatPrior((0.0, 1.0)), P.GaussianPrior(0.0, 1.0)],
                                    [[P.FlatPrior((0.0, 1.0)), link(-100.0, 100.0, 0, 37.4, 0.01, 1.0, pivot=0.5)],
                                     [P.FlatPrior((0.0, 1.0)), link(-100.0, 100.0, 0, 20.0, 0.5, 1.0, pivot=0.5)]], W, T)
    return out


def check_special(name, case, g):
    """What the special case ``name`` must show in the results ``g`` beyond matching the twin."""
    if name == "parent_nan":
        assert list(g["n_bad"]) == [1, 0, 2] and np.isfinite(g["ell"]).all()
    elif name == "child_out":
        assert np.isneginf(g["ell"][:, 1]).all() and (g["ess"][:, 1] == 0.0).all() and np.isfinite(g["ell"][:, [0, 2]]).all()
        assert list(g["n_bad"]) == [0, 0, 0] and np.isneginf(g["L"]).all()
    elif name == "mean_60_sigma":
        assert np.isneginf(g["ell"][0]).all() and (g["ess"][0] == 0.0).all() and np.isfinite(g["ell"][1]).all()
    elif name == "bad_parent":
        assert np.isneginf(g["ell"][:3]).all() and (g["ess"][:3] == 0.0).all() and np.isfinite(g["ell"][3]).all()
        assert list(g["n_bad"]) == [0, 0, 0]
    elif name == "masked":
        assert np.isnan(g["ell"][:, 1]).all() and np.isnan(g["ess"][:, 1]).all() and g["n_bad"][1] == 0
        assert np.isfinite(g["L"]).all() and np.isfinite(g["min_ess"]).all()
    else:
        assert want(case)["rmax"].max() > 690 and np.isfinite(g["ell"]).all() and np.isfinite(g["ess"]).all()


def slope_zero_pair(S=3, W=40, T=30, H=hc.ROW_TILE + 1, seed=4):
    """``(linked, plain)``: the same chains, column 1 LINGAUSS with slope 0 on column 0 and the TRUNCGAUSS it then is."""
    plain = tw.random_case(S, W, T, 2, H, seed=seed)                # seed 4: column 0 mass (a power law), column 1 [Fe/H]
    assert (plain["rows"][:, 1]["kind"] == hc.TRUNCGAUSS).all()
    rows = plain["rows"].copy()
    for h in range(H):
        tg = rows[h, 1]
        rows[h, 1] = link(float(tg["lo"]), float(tg["hi"]), 0, float(tg["p"][0]), 0.0, float(tg["p"][1]), pivot=1.0)[0]
    return dict(plain, rows=rows), plain


# -- the closed-form case ---------------------------------------------------------------------------------------------
def closed_form_case(seed=2):
    """200 stars, W = 32, T = 64.  Truth x ~ N(9.6, 0.3), y | x ~ N(-0.1 + 0.5 (x - 9.6), 0.15); both observed with error
    0.1; the chains are independent draws N(observed, 0.1) (the posterior under a flat interim prior); interims flat on
    (5, 14) and (-6, 6).  Rows: the slope grid (0, 0.25, 0.5, 0.75, 1) at the true other parameters.  ``exact`` [H, S]:
    ln of the bivariate normal density of (x_obs, y_obs) with mean (9.6, -0.1 + b * 0) and covariance [[sx^2 + ex^2,
    b sx^2], [b sx^2, b^2 sx^2 + sg^2 + ey^2]], plus ln 9 + ln 12 for the flat interim density."""
    rng = np.random.default_rng(seed)
    S, W, T = 200, 32, 64
    M = W * T
    sx, sg, e, b0, mx = 0.3, 0.15, 0.1, -0.1, 9.6
    xt = rng.normal(mx, sx, S)
    yt = rng.normal(b0 + 0.5 * (xt - mx), sg)
    xo, yo = xt + rng.normal(0.0, e, S), yt + rng.normal(0.0, e, S)
    x = np.stack([xo[:, None] + rng.normal(0.0, e, (S, M)), yo[:, None] + rng.normal(0.0, e, (S, M))])
    slopes = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    model = hi.PopulationModel(x=hi.TruncatedGaussian((5.0, 14.0)), y=relations.LinearGaussian("x", (-6.0, 6.0), (-2.0, 2.0), pivot=mx))
    theta = np.column_stack([np.full(5, mx), np.full(5, sx), np.full(5, b0), slopes, np.full(5, sg)])
    rows = model.pack(theta)
    interim = np.concatenate([hi.prior_record(P.FlatPrior((5.0, 14.0))), hi.prior_record(P.FlatPrior((-6.0, 6.0)))])
    storages, where = tw.place(x, W, T, _cabi.CHAIN_PARAM_MAJOR, seed)
    exact = np.empty((5, S))
    for h, b in enumerate(slopes):
        cov = np.array([[sx * sx + e * e, b * sx * sx], [b * sx * sx, b * b * sx * sx + sg * sg + e * e]])
        d = np.stack([xo - mx, yo - b0])
        quad = np.einsum("is,ij,js->s", d, np.linalg.inv(cov), d)
        exact[h] = -0.5 * quad - np.log(2 * np.pi) - 0.5 * np.log(np.linalg.det(cov)) + np.log(9.0) + np.log(12.0)
    case = dict(x=x, interim=interim, rows=rows, storages=storages, where=where, S=S, W=W, T=T,
                layout=_cabi.CHAIN_PARAM_MAJOR, mask=None)
    return case, exact, slopes, model, theta


def check_closed_form(got, exact, slopes, M):
    """Every star within 5 standard errors of the exact ell, se = sqrt(1 / ess - 1 / M); L peaks at slope 0.5."""
    se = np.sqrt(1.0 / got["ess"] - 1.0 / M)
    dev = np.abs(got["ell"] - exact) / se
    print("closed form: worst star %.2f se, L = %s" % (dev.max(), np.array2string(got["L"], precision=2)))
    assert np.all(dev <= 5.0), float(dev.max())
    assert slopes[int(np.argmax(got["L"]))] == 0.5


# -- the call ---------------------------------------------------------------------------------------------------------
class _AsHier:
    """libiso_relation.so's two likelihood entries under the names _hier_twin.call looks up: the argument lists are equal."""

    def __init__(self, lib):
        self.iso_hier_lnlike, self.iso_hier_lnlike_host = lib.iso_relation_lnlike, lib.iso_relation_lnlike_host


def call(lib, case, **kw):
    """_hier_twin.call on ``iso_relation_lnlike_host`` or, with ``device``, ``iso_relation_lnlike``."""
    return tw.call(_AsHier(lib), case, **kw)
