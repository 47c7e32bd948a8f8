"""The definition of include/isochrones_amd_population.h in numpy: every product and every sum one float64 numpy
operation in the header's order (the interpolation is the derived and the predictive twin's), and the fixtures and the
ctypes calls the host-ABI, the golden and the GPU tests share."""
import ctypes as C
import functools
import os

import numpy as np

from tests._derived_twin import interp as interp3, same_bits  # noqa: F401
from tests._predict_twin import interp4

TOL = 1e-9           # |a - b| <= TOL * max(1, |b|): the tolerance the project's tests hold between two math libraries
SENTINEL = -7.0
QS = (4, 5, 8, 9, 18)
BS = (1, 3, 7)
NS = (1, 2, 63, 64, 65, 257, 1000)
#: (Q, B) beyond the tables' own 18 columns and 7 bands: three and four full groups of the column walk, a remainder of seven,
#: one, two, three and four passes of eight bands, a last pass of one, both limits
WIDE = ((24, 8), (31, 9), (18, 17), (32, 32))
OUTPUTS = ("cols_out", "mag_out", "A_out", "sys_mag", "sys_A")


def evaluate(tab, coords, dist, av):
    """tab = (cols [n0, n1, nk, Q], axes3, hot, bc [.., B], axes4); coords [C, 3, N]; dist, av [N] -> dict of the
    header's outputs: cols_out [C, Q, N], mag_out, A_out [C, B, N], sys_mag, sys_A [B, N]."""
    cols, axes3, hot, bc, axes4 = tab
    Cn, _, N = coords.shape
    Q, B = cols.shape[3], bc.shape[4]
    out = dict(cols_out=np.empty((Cn, Q, N)), mag_out=np.empty((Cn, B, N)), A_out=np.empty((Cn, B, N)))
    with np.errstate(all="ignore"):
        dm = 5 * np.log10(dist / 10.0)
        for c in range(Cn):
            v = interp3(cols, axes3, coords[c, 0], coords[c, 1], coords[c, 2])              # [N, Q]
            teff, logg, feh, mbol = (v[:, h] for h in hot)
            b1 = interp4(bc, axes4, [teff, logg, feh, av])
            b0 = interp4(bc, axes4, [teff, logg, feh, np.zeros(N)])
            base = (mbol + dm)[:, None]
            mag, tru = base - b1, base - b0
            out["cols_out"][c], out["mag_out"][c], out["A_out"][c] = v.T, mag.T, (mag - tru).T
        m0, a0 = out["mag_out"][0], out["A_out"][0]
        if Cn == 1:
            out["sys_mag"], out["sys_A"] = m0.copy(), a0.copy()
        else:
            m1 = np.where(np.isnan(out["mag_out"][1]), np.inf, out["mag_out"][1])
            a1 = np.where(np.isnan(out["A_out"][1]), 0.0, out["A_out"][1])
            sm = -2.5 * np.log10((0.0 + np.power(10.0, -0.4 * m0)) + np.power(10.0, -0.4 * m1))
            st = -2.5 * np.log10((0.0 + np.power(10.0, -0.4 * (m0 - a0))) + np.power(10.0, -0.4 * (m1 - a1)))
            out["sys_mag"], out["sys_A"] = sm, sm - st
    return out


def close(a, b, tol=TOL):
    """NaN and infinity positions identical, |a - b| <= tol * max(1, |b|) elsewhere -> (ok, largest deviation in that measure)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False, np.inf
    fin = np.isfinite(b)
    if not np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]):
        return False, np.inf
    dev = float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin])))) if fin.any() else 0.0
    return dev <= tol, dev


def assert_same(got, want, what=""):
    """Model columns bit for bit; magnitudes and extinctions within TOL with the same NaN pattern."""
    assert same_bits(got["cols_out"], want["cols_out"]), what + " cols_out"
    for k in OUTPUTS[1:]:
        ok, dev = close(got[k], want[k])
        assert ok, (what, k, dev)


# ---- fixtures ------------------------------------------------------------------------------------------------------------

#: the nodes of the test table (feh index 2, mass index 3, EEP index 5 + j) whose Teff, logg or feh is set to a value on or
#: one ulp outside an axis of the BC table: (hot column, which value of that axis)
_POKES = [(h, k) for h in range(3) for k in ("first", "last", "below", "above")]
_POKE_NODE = (2, 3, 5)


def _poke_value(ax, k):
    return {"first": ax[0], "last": ax[-1], "below": np.nextafter(ax[0], -np.inf), "above": np.nextafter(ax[-1], np.inf)}[k]


@functools.lru_cache(maxsize=None)
def tables(Q=18, B=7):
    """(cols [5, 10, 48, Q], axes3, hot, bc [5, 5, 6, 4, B], axes4) of the small track and BC tables of oracle/make_golden,
    read-only.  For Q < 18 the columns are logg, Mbol, the first Q - 4 others, feh, Teff: the hot four sit in the first and
    in the last group of the kernel's column walk; beyond 18 columns or 7 bands (the tables have no more) the columns repeat,
    shifted: tables for the C ABI alone.  Twelve nodes carry a Teff, logg or feh exactly on the first or the last
    node of its BC axis or one ulp outside it (:data:`_POKES`); a query on such a node returns that value exactly."""
    from oracle import make_golden as mg
    g, ax, names = mg.small_track()
    bg, bax, bands = mg.small_bc()
    names = list(names)
    hot_full = [names.index(n) for n in ("Teff", "logg", "feh", "Mbol")]
    if Q >= len(names):                                         # beyond 18: the columns again (shifted below)
        order = [j % len(names) for j in range(Q)]
    else:
        others = [i for i in range(len(names)) if i not in hot_full]
        order = [hot_full[1], hot_full[3]] + others[:Q - 4] + [hot_full[2], hot_full[0]]
    cols = np.ascontiguousarray(g[..., order], dtype=np.float64)
    cols[..., len(names):] += 0.5
    hot = tuple(order.index(i) for i in hot_full)
    ax4 = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in bax)
    i, j, k = _POKE_NODE
    for n, (h, which) in enumerate(_POKES):
        cols[i, j, k + n, hot[h]] = _poke_value(ax4[h], which)
    nb = len(bands)                                             # beyond 7 bands: column j is column j mod 7 shifted by 0.01 (j div 7)
    bc = np.ascontiguousarray(np.stack([bg[..., j % nb] + 0.01 * (j // nb) for j in range(B)], axis=-1), dtype=np.float64)
    ax3 = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in ax)
    for a in (cols, bc):
        a.setflags(write=False)
    return cols, ax3, hot, bc, ax4


def edge_rows(tab):
    """Rows (x0, x1, xk of the primary; x0, x1, xk of the secondary; distance, AV) that every batch of the tests starts
    with: an absent secondary, every model axis on its first and last node and one ulp outside, the poked nodes (the BC
    axes T, g, f on and off their ends), AV on 0, on the last node and one ulp outside, a Teff beyond the BC table, a NaN in
    every input."""
    _, ax3, _, _, ax4 = tab
    f, m, e = ax3
    good = [f[2] + 0.1, 0.85, e[10] + 0.3]
    sec = [f[2] + 0.1, 0.62, e[7] + 0.6]
    rows = [good + sec + [120.0, 0.25],
            good + [f[2] + 0.1, 0.0, np.nan] + [120.0, 0.25]]                                # mass_B = 0
    for a, ax in enumerate(ax3):
        for x in (ax[0], ax[-1], np.nextafter(ax[0], -np.inf), np.nextafter(ax[-1], np.inf), np.nan):
            p = list(good)
            p[a] = x
            if a == 1 and x == ax[-1]:
                p[2] = e[3]                                                                  # (the 8 Msun track is short)
            rows.append(p + sec + [200.0, 0.3])
            rows.append(good + p + [200.0, 0.3])
    i, j, k = _POKE_NODE
    for n in range(len(_POKES)):
        node = [f[i], m[j], e[k + n]]
        rows.append(node + sec + [80.0, 0.05])
        rows.append(good + node + [80.0, 0.7])
    A = ax4[3]
    for av in (0.0, A[-1], np.nextafter(A[-1], np.inf), -5e-324, -0.0, A[1], np.nan):
        rows.append(good + sec + [150.0, av])
    rows.append(good + sec + [np.nan, 0.2])
    cols, hot = tab[0], tab[2]
    k = int(np.nanargmax(cols[3, -1, :, hot[0]]))                                            # Teff beyond the BC table
    rows.append([f[3], m[-1], e[k]] + sec + [100.0, 0.2])
    rows.append(good + [f[3], m[-1], e[k]] + [100.0, 0.2])
    return np.array(rows, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def inputs(N, Cn, seed=0):
    """(coords [Cn, 3, N], distance [N], AV [N]) over :func:`tables`: the first rows are :func:`edge_rows`, the others
    uniform over the cool part of the table with one secondary in five absent.  Read-only."""
    tab = tables()
    _, (f, m, e), _, _, ax4 = tab
    rng = np.random.default_rng(100 * N + Cn + seed)
    rows = np.empty((N, 8))
    rows[:, 0] = rows[:, 3] = rng.uniform(f[0], f[-1], N)
    rows[:, 1] = rng.uniform(0.5, 1.6, N)
    rows[:, 4] = np.where(rng.integers(0, 5, N) == 0, 0.0, rows[:, 1] * rng.uniform(0.2, 1.0, N))
    rows[:, 2] = rng.uniform(e[0], e[-1], N)
    rows[:, 5] = np.where(rows[:, 4] == 0.0, np.nan, rng.uniform(e[0], e[-1], N))
    rows[:, 6] = rng.uniform(10.0, 2000.0, N)
    rows[:, 7] = rng.uniform(0.0, ax4[3][-1], N)
    edges = edge_rows(tab)
    n = min(N, len(edges))
    rows[:n] = edges[:n]
    coords = np.ascontiguousarray(rows[:, :3 * Cn].T.reshape(Cn, 3, N))
    dist, av = np.ascontiguousarray(rows[:, 6]), np.ascontiguousarray(rows[:, 7])
    for a in (coords, dist, av):
        a.setflags(write=False)
    return coords, dist, av


# ---- the C ABI on numpy arrays ---------------------------------------------------------------------------------------------

def shapes(Cn, Q, B, N):
    return dict(cols_out=(Cn, Q, N), mag_out=(Cn, B, N), A_out=(Cn, B, N), sys_mag=(B, N), sys_A=(B, N))


def structs(pc, ptr, tab):
    cols, ax3, hot, bc, ax4 = tab
    mt = pc.IsoPopulationModelTable(ptr(cols), ptr(ax3[0]), ptr(ax3[1]), ptr(ax3[2]), *cols.shape[:4],
                                    (C.c_int32 * 4)(*hot))
    bt = pc.IsoPopulationBcTable(ptr(bc), *[ptr(a) for a in ax4], *bc.shape[:5], 0)
    return mt, bt


def host(tab, coords, dist, av, want=None, rc_only=False, N=None, Cn=None):
    """iso_population_eval_host on numpy arrays -> dict of outputs, every one filled with SENTINEL before the call (or the
    return code with ``rc_only``).  ``want``: the outputs asked for (the others get a null pointer)."""
    from isochrones_amd import _population_cabi as pc
    p = lambda a: None if a is None else a.ctypes.data                          # noqa: E731
    Cn = coords.shape[0] if Cn is None else Cn
    N = coords.shape[2] if N is None else N
    mt, bt = structs(pc, p, tab)
    o = {k: np.full(tuple(max(n, 1) for n in s), SENTINEL)
         for k, s in shapes(max(Cn, 1), tab[0].shape[3], tab[3].shape[4], max(N, 1)).items()}
    out = pc.IsoPopulationOut(*[p(o[k]) if want is None or k in want else None for k in OUTPUTS])
    rc = pc.lib().iso_population_eval_host(C.byref(mt), C.byref(bt), p(coords), p(dist), p(av), N, Cn, C.byref(out), None)
    if rc_only:
        return rc
    assert rc == 0, pc.lib().iso_population_last_error()
    return o


class DeviceTables:
    """The tables of :func:`tables` on the current device, and the two structs that point at them."""

    def __init__(self, tab):
        import torch
        from isochrones_amd import _population_cabi as pc
        cols, ax3, hot, bc, ax4 = tab
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
        self.keep = (up(cols), tuple(up(a) for a in ax3), hot, up(bc), tuple(up(a) for a in ax4))
        self.Q, self.B = cols.shape[3], bc.shape[4]
        self.model, self.bct = structs(pc, lambda t: t.data_ptr(), self.keep)


MARGIN = 64


def guarded(shape):
    """A float64 CUDA tensor of ``shape`` filled with SENTINEL, inside a buffer with MARGIN sentinels either side of it."""
    import torch
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.float64, device="cuda")
    return flat, flat[MARGIN:MARGIN + n].view(shape)


def margins_untouched(flat):
    return bool((flat[:MARGIN] == SENTINEL).all()) and bool((flat[-MARGIN:] == SENTINEL).all())


def device(dt, coords, dist, av, want=None, stream=None):
    """iso_population_eval on host arrays copied to the device -> dict of numpy outputs.  Every output lies between two
    margins of SENTINEL that have to stay so; an output not in ``want`` gets a null pointer."""
    return {k: view.cpu().numpy() for k, view in device_tensors(dt, coords, dist, av, want, stream).items()}


def device_tensors(dt, coords, dist, av, want=None, stream=None):
    """:func:`device` with the outputs left on the device (a large batch is compared there, or on windows)."""
    import torch
    from isochrones_amd import _population_cabi as pc, device as dev
    Cn, _, N = coords.shape
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")      # noqa: E731
    d_x, d_d, d_a = up(coords), up(dist), up(av)
    bufs = {k: guarded(s) for k, s in shapes(Cn, dt.Q, dt.B, N).items()}
    out = pc.IsoPopulationOut(*[dev.ptr(bufs[k][1]) if want is None or k in want else None for k in OUTPUTS])
    pc.check(pc.lib().iso_population_eval(C.byref(dt.model), C.byref(dt.bct), dev.ptr(d_x), dev.ptr(d_d), dev.ptr(d_a), N, Cn,
                                          C.byref(out), dev.stream_ptr(0) if stream is None else stream))
    torch.cuda.synchronize()
    for k, (flat, _) in bufs.items():
        assert margins_untouched(flat), "the kernel wrote outside " + k
    return {k: view for k, (_, view) in bufs.items()}


# ---- the Python layer without a device --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_ic():
    """The project's track interpolator over the small tables of oracle/make_golden (18 columns, 7 bands)."""
    import isochrones_amd as ia
    from isochrones_amd import models
    from oracle import make_golden as mg
    g, ax, names = mg.small_track()
    bg, bax, bands = mg.small_bc()
    grid = models.EvolutionTrackGrid(ia.DFInterpolator.from_arrays(g, ax, names, ["initial_feh", "initial_mass", "EEP"]),
                                     limits=mg.limits_of("track", ax))
    bc = models.BolometricCorrectionGrid(ia.DFInterpolator.from_arrays(bg, bax, bands, ["Teff", "logg", "[Fe/H]", "Av"]),
                                         bands=bands)
    return models.EvolutionTrackInterpolator(grid, bc, bands=bands, eep_bounds=(ax[2][0], ax[2][-1]))


def host_backend():
    """The host backend of populations.py with the EEP estimate of the C oracle (``orc_interp_eep``, the reference's
    ``interp_eeps``) in the place of the device path ``ic.get_eep``."""
    from isochrones_amd import populations as pp
    from isochrones_amd.ingest import ragged_age_arrays
    from oracle import oracle as orc

    class Backend(pp._HostBackend):
        def eep(self, ic, mass, age, feh, accurate):
            dfi = ic.model_grid.interp
            ages, lengths = ragged_age_arrays(dfi, "age")
            fehs, masses, eeps = dfi.index_columns
            # (interp_eeps counts EEPs from 1: the table's first EEP is added, as tools/make_solve_golden.py does)
            return orc.interp_eep(age, feh, mass, fehs, masses, ages, lengths) + (eeps[0] - 1.0)

    return Backend()


# ---- the golden from the reference -------------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "population", "binary.npz")


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check_against_golden(g, backend):
    """``populations._evaluate`` on the golden's inputs and EEPs through ``backend``, compared column by column."""
    from isochrones_amd import populations as pp
    got = pp._evaluate(small_ic(), g["mass_A"], g["mass_B"], g["age"], g["feh"], g["distance"], g["AV"], None, "all", False,
                       (g["eep_A"], g["eep_B"]), backend)
    assert got.columns == [str(c) for c in g["columns"]]
    m = np.asarray(backend.to_host(got.matrix))
    worst = 0.0
    for r, c in enumerate(got.columns):
        ok, dev = close(m[r], g["values"][:, r])
        assert ok, (c, dev)
        worst = max(worst, dev)
    return worst
