"""numpy twin of libiso_draw.so: the definition of include/isochrones_amd_draw.h restated on packed records, the uniforms from
oracle.cpu_sampler.philox4x32_10 (the samplers' own twin of the generator), the maps in numpy long double with
scipy.special.ndtri and scipy.special.erfc at float64 (scipy has neither in long double)."""
import numpy as np
from scipy import special, stats

from isochrones_amd import _draw_cabi as dc, draws, priors as P
from oracle.cpu_sampler import philox4x32_10

LD = np.longdouble
M21 = np.uint64(0x1FFFFF)


def _u53(hi, lo):
    m = (hi.astype(np.uint64) << np.uint64(21)) | (lo.astype(np.uint64) & M21)
    u = (m.astype(np.float64) + 0.5) * 2.0 ** -53
    return np.where(u < 1.0, u, 1.0 - 2.0 ** -53)


def uniforms(seed, j, stream, rnd):
    """[n, 2]: (u0, u1) of the systems j (int64; read as uint64)."""
    j = np.asarray(j, dtype=np.int64).astype(np.uint64)
    c2 = np.full(j.shape, (int(stream) | (int(rnd) << 8)) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(j.shape, dc.PHILOX_TAG, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), c2, c3, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([_u53(w[0], w[1]), _u53(w[2], w[3])], axis=1)


def _ndtri(p):
    return special.ndtri(np.asarray(p, dtype=np.float64)).astype(LD)


def _phi(z):
    return (0.5 * special.erfc(-np.asarray(z, dtype=np.float64) / np.sqrt(2.0))).astype(LD)


def _plaw(u, a1, E, base, hi, mode):
    if mode == 1:
        return base * np.exp(u * E)
    if mode == 2:
        return hi * np.exp(np.log(u) / a1)
    return base * np.exp(np.log1p(u * E) / a1)


def _bracket(edges, x):
    return np.clip(np.searchsorted(edges, np.asarray(x, dtype=np.float64), side="right") - 1, 0, len(edges) - 2)


def draw_column(R, u0, u1, xp, tables, choice=None):
    """The long-double value of every system for the record R; ``choice`` (a list) receives the discrete choice."""
    p = [LD(v) for v in R["p"]]
    lo, hi = LD(R["lo"]), LD(R["hi"])
    u0, u1 = u0.astype(LD), u1.astype(LD)
    kind = int(R["kind"])
    pick = None
    with np.errstate(all="ignore"):
        if kind == dc.FLAT:
            v = lo + u0 * (hi - lo)
        elif kind == dc.FLATLOG:
            v = np.log10(u0 * p[1] + p[0])
        elif kind == dc.POWERLAW:
            v = _plaw(u0, p[0], p[1], lo, hi, int(p[2]))
        elif kind in (dc.GAUSS, dc.TRUNCGAUSS):
            z = _ndtri(p[2] + u0 * p[3])
            v = p[0] + p[1] * (-z if p[4] != 0 else z)
        elif kind == dc.LOGNORMAL:
            v = np.exp(p[0] + p[1] * _ndtri(u0))
        elif kind == dc.CHABRIER:
            w = p[0]
            pick = (u0 >= w).astype(int)
            z = _ndtri(p[3] + (u0 / (w if w > 0 else LD(1))) * p[4])
            low = np.exp(p[1] + p[2] * (-z if p[5] != 0 else z))
            high = _plaw((u0 - w) / ((1 - w) if w < 1 else LD(1)), p[6], p[7], p[8], hi, int(p[9]))
            v = np.where(pick == 0, low, high)
        elif kind == dc.FEH:
            local = p[0] != 0
            pick = np.where(u0 < p[1], 0, np.where(u0 < p[2], 1, 2))
            halo = pick == (2 if local else 1)
            mu = np.where(halo, LD(-1.5), np.where(pick == 0, LD(0.016), LD(-0.15)) if local else LD(-0.3))
            sg = np.where(halo, LD(0.4), np.where(pick == 0, LD(0.15), LD(0.22)) if local else LD(0.3))
            # the constants are float64 literals in the definition
            mu, sg = mu.astype(np.float64).astype(LD), sg.astype(np.float64).astype(LD)
            fa = np.choose(pick, [p[3], p[5], p[7]])
            df = np.choose(pick, [p[4], p[6], p[8]])
            flip = (int(p[9]) >> pick) & 1
            z = _ndtri(fa + u1 * df)
            v = mu + sg * np.where(flip != 0, -z, z)
        elif kind == dc.LINGAUSS:
            xp = xp.astype(LD)
            mu = p[0] + p[4] * (xp - p[5])
            a, b = (lo - mu) * p[3], (hi - mu) * p[3]
            flip = a > 0
            a, b = np.where(flip, -b, a), np.where(flip, -a, b)
            fa, fb = _phi(a), _phi(b)
            z = _ndtri(fa + u0 * (fb - fa))
            v = mu + p[1] * np.where(flip, -z, z)
            v = np.where(fb - fa > 0, v, np.where(np.isnan(fb - fa), LD(np.nan), np.where(flip, lo, hi)))
        elif kind == dc.TABLE:
            off, K, Kp, poff = int(p[0]), int(p[1]), int(p[2]), int(p[3])
            e = tables[off:off + K + 1].astype(LD)
            row = _bracket(tables[poff:poff + Kp + 1], xp) if Kp > 0 else np.zeros(u0.shape, dtype=int)
            cum = tables[off + K + 1:off + (K + 1) * (1 + max(Kp, 1))].reshape(max(Kp, 1), K + 1)
            c = cum[row]                                                     # [n, K + 1]
            k = np.sum(np.asarray(u0, dtype=np.float64)[:, None] >= c[:, 1:K], axis=1)
            pick = k + K * row
            n = np.arange(u0.size)
            c0, c1 = c[n, k].astype(LD), c[n, k + 1].astype(LD)
            v = e[k] + (u0 - c0) / (c1 - c0) * (e[k + 1] - e[k])
        elif kind == dc.CONSTANT:
            v = np.full(u0.shape, p[0], dtype=LD)
        else:
            raise ValueError("unknown kind %d" % kind)
    if choice is not None:
        choice.append(pick)
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def draw(records, order, tables, seed, rnd, first, index, N, choices=None):
    """x [C, N] in long double: iso_draw_systems_host's arguments.  ``choices`` (a dict) receives {column: discrete choice}."""
    C_ = len(records)
    order = list(range(C_)) if order is None else [int(q) for q in order]
    j = np.asarray(index, dtype=np.int64) if index is not None else np.int64(first) + np.arange(N, dtype=np.int64)
    x = np.zeros((C_, N), dtype=LD)
    for q in order:
        R = records[q]
        u = uniforms(seed, j, int(R["stream"]), rnd)
        got = []
        x[q] = draw_column(R, u[:, 0], u[:, 1], x[int(R["parent"])] if int(R["parent"]) >= 0 else None, tables, got)
        if choices is not None:
            choices[q] = got[0]
    return x


# ---- the plans and the measures the CPU and the GPU tests share ---------------------------------------------------------------

TOL = 1e-11
#: kinds whose values are positive: the bound is relative; for the location-scale kinds it is relative to max(1, |x|)
POSITIVE = (dc.POWERLAW, dc.LOGNORMAL, dc.CHABRIER)


def host(plan, n, seed, rnd=0, first=0, index=None):
    x = np.full((len(plan.records), n), np.nan)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64)
    dc.check(dc.lib().iso_draw_systems_host(plan.records.ctypes.data, len(plan.records), plan.order.ctypes.data,
                                            plan.tables.ctypes.data if plan.tables.size else None, plan.tables.size, seed, rnd,
                                            first, None if idx is None else idx.ctypes.data, n, x.ctypes.data, None))
    return x


def error(plan, got, ref):
    """The largest error over the columns, each in its kind's measure."""
    worst = 0.0
    for q, R in enumerate(plan.records):
        d = np.abs(got[q].astype(np.longdouble) - ref[q])
        scale = np.abs(ref[q]) if int(R["kind"]) in POSITIVE else np.maximum(1.0, np.abs(ref[q]))
        worst = max(worst, float(np.max(d / scale)))
    return worst


def edges_masses(K, rng, rows=None):
    e = np.cumsum(rng.uniform(0.1, 1.0, K + 1)) - 3.0
    m = rng.uniform(0.0, 1.0, (rows or 1, K))
    if K > 3:
        m[:, 1] = 0.0                                                # an empty bin is never drawn
    return e, (m if rows else m[0])


def every_kind():
    """Eight columns: every kind but TABLE and LINGAUSS's chain (eight is the limit; the others follow)."""
    return {"flat": P.FlatPrior((-2.0, 3.0)), "age": P.FlatLogPrior((5.0, 10.15)), "q": P.PowerLawPrior(0.3, (0.2, 1.0)),
            "g": P.GaussianPrior(1.0, 2.0), "tg": P.GaussianPrior(0.0, 1.0, bounds=(-0.5, 2.5)),
            "ln": P.LogNormalPrior(0.2, 0.6), "imf": P.ChabrierPrior(), "feh": P.FehPrior()}


def linked():
    rng = np.random.default_rng(11)
    e1, m1 = edges_masses(1, rng)
    e64, m64 = edges_masses(64, rng)
    pe, pm = edges_masses(3, rng)
    ce, cm = edges_masses(4, rng, rows=3)
    # child before its parent (index 0 follows index 2), a chain of two links (0 -> 2 -> 3), a conditional table of 3 x 4 bins
    return {"c2": draws.lingauss("c1", (-4.0, 4.0), 0.1, -0.7, 0.5, pivot=1.0), "k1": draws.table(e1, m1),
            "c1": draws.lingauss("root", (-1.0, 6.0), 2.0, 1.5, 0.8), "root": P.FlatPrior((-1.0, 1.0)),
            "k64": draws.table(e64, m64), "par": draws.table(pe, pm), "kid": draws.table(ce, cm, given="par", parent_edges=pe),
            "const": 2.5}


def edge_cases():
    return {"tg_lo": draws.truncgauss(-30.0, 1.0, (0.0, 1.0)), "tg_hi": draws.truncgauss(31.0, 1.0, (0.0, 1.0)),
            "pl_m1": draws.powerlaw(-1.0, (0.1, 10.0)), "pl_m1p": draws.powerlaw(-1.0 + 1e-9, (0.1, 10.0)),
            "pl_m1m": draws.powerlaw(-1.0 - 1e-9, (0.1, 10.0)), "sfh": stats.uniform(0, 10), "dist": P.DistancePrior(3000.0),
            "feh_nl": P.FehPrior(halo_fraction=0.2, local=False, bounds=(-2.0, 0.2))}


def far_links():
    """LINGAUSS whose mean lies 60 sigma below and above its bounds (the window's mass underflows at the sample: the bound
    next to the mean) and 30 sigma outside (a mass of 1e-198: drawn)."""
    return {"par": P.FlatPrior((0.0, 1.0)), "below": draws.lingauss("par", (0.0, 1.0), -60.0, 1.0, 1.0),
            "above": draws.lingauss("par", (0.0, 1.0), 61.0, 1.0, 1.0), "low30": draws.lingauss("par", (0.0, 1.0), -30.0, 0.5, 1.0),
            "high30": draws.lingauss("par", (0.0, 1.0), 31.0, 0.5, 1.0)}


PLANS = {"kinds": every_kind, "linked": linked, "edges": edge_cases, "far": far_links}


def feh_component(R, u1, x):
    """The FEH component a drawn value x came from: the one whose inverse of u1 it is (the nearest of the two or three
    candidates; they are apart by the components' different means and widths)."""
    p = R["p"]
    local = p[0] != 0
    comps = [(0.016, 0.15), (-0.15, 0.22), (-1.5, 0.4)] if local else [(-0.3, 0.3), (-1.5, 0.4)]
    cand = []
    for k, (m, s) in enumerate(comps):
        z = special.ndtri(p[3 + 2 * k] + u1 * p[4 + 2 * k])
        cand.append(np.clip(m + s * (-z if (int(p[9]) >> k) & 1 else z), R["lo"], R["hi"]))
    return np.argmin(np.abs(np.asarray(cand) - np.asarray(x, dtype=np.float64)[None, :]), axis=0)
