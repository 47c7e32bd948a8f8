"""Synthetic stellar populations (reference: isochrones/populations.py): ``StarPopulation`` draws primaries from an IMF,
companions from a binary fraction and a mass-ratio law, ages from a star-formation history and [Fe/H] from a prior, and
evaluates all systems in one launch of the HIP kernel of libiso_population.so (``iso_population_eval``; the definition
is in include/isochrones_amd_population.h): per component the model columns, the magnitudes and the per-band
extinctions, per system the combined magnitudes and extinctions - the reference's ``generate_binary(..., all_As=True)``.
The draws are made on the host with one seeded ``numpy.random.Generator`` or, with ``rng="philox"``, where the systems are
evaluated by libiso_draw.so (:mod:`isochrones_amd.draws`); the EEPs come from the device paths that exist (``ic.get_eep`` /
``ic.solve_eep`` on CUDA tensors)."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _chain, _population_cabi, _tables, device as dev
from .priors import ChabrierPrior, FehPrior, PowerLawPrior

#: how often ``StarPopulation.generate(exact_N=True)`` redraws the rows that fell off the grid before it gives up
MAX_REDRAW_ROUNDS = 100


# ---- where the arrays live: the device (the product) or the host (the *_host entry point; the CPU tests) --------------------

class _DeviceBackend:
    """CUDA tensors on one device; EEPs from ``ic.get_eep`` / ``ic.solve_eep``, the evaluation by ``iso_population_eval`` on
    the current stream."""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, int(device)

    def array(self, x):
        return dev.to_device_f64(x, self.device)

    def broadcast(self, xs):
        return [t.reshape(-1).contiguous() for t in self.torch.broadcast_tensors(*[self.array(x) for x in xs])]

    def empty(self, *shape):
        return dev.empty_f64(shape, self.device)

    def cat(self, xs):
        return self.torch.cat(list(xs), dim=0)

    def stack(self, xs, axis=0):
        return self.torch.stack(list(xs), dim=axis)

    def isnan(self, x):
        return self.torch.isnan(x)

    def take(self, m, keep):
        return m[:, keep]

    def any(self, mask):
        return bool(mask.any())

    def count(self, mask):
        return int(mask.sum())

    def to_host(self, x):
        return x.cpu().numpy()

    def ptr(self, x):
        return dev.ptr(x)

    def eep(self, ic, mass, age, feh, accurate):
        return ic.solve_eep(mass, age, feh) if accurate else ic.get_eep(mass, age, feh)

    def call(self, tables, coords, dist, av, N, Cn, out):
        with self.torch.cuda.device(self.device):
            _population_cabi.check(_population_cabi.lib().iso_population_eval(
                C.byref(tables.model), C.byref(tables.bct), self.ptr(coords), self.ptr(dist), self.ptr(av), N, Cn,
                C.byref(out), dev.stream_ptr(self.device)))


class _HostBackend:
    """numpy arrays and ``iso_population_eval_host``: no device is touched.  It has no EEP estimate of its own (the
    project's are device paths): pass ``eeps``, or subclass and give ``eep``."""
    device = "host"

    def array(self, x):
        return np.ascontiguousarray(x, dtype=np.float64)

    def broadcast(self, xs):
        return [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in np.broadcast_arrays(*[np.atleast_1d(x) for x in xs])]

    def empty(self, *shape):
        return np.empty(shape)

    def cat(self, xs):
        return np.concatenate(list(xs), axis=0)

    def stack(self, xs, axis=0):
        return np.stack(list(xs), axis=axis)

    def isnan(self, x):
        return np.isnan(x)

    def take(self, m, keep):
        return np.ascontiguousarray(m[:, keep])

    def any(self, mask):
        return bool(mask.any())

    def count(self, mask):
        return int(mask.sum())

    def to_host(self, x):
        return x

    def ptr(self, x):
        return C.c_void_p(x.ctypes.data)

    def eep(self, ic, mass, age, feh, accurate):
        raise NotImplementedError("the host backend has no EEP estimate: pass eeps=(eep_A, eep_B)")

    def call(self, tables, coords, dist, av, N, Cn, out):
        _population_cabi.check(_population_cabi.lib().iso_population_eval_host(
            C.byref(tables.model), C.byref(tables.bct), self.ptr(coords), self.ptr(dist), self.ptr(av), N, Cn,
            C.byref(out), None))


class PopulationTables:
    """The ``cols`` columns of the model grid packed ``[n0, n1, nk, Q]`` (the hot four among them) and the ``bands`` columns
    of the BC grid packed ``[nT, ng, nf, nA, B]`` where a backend keeps its arrays, with their axes and the two structs."""

    def __init__(self, ic, cols, bands, backend):
        m = ic.model_grid.interp
        names = list(m.columns)
        icols = [names.index(c) for c in cols]
        self.cols, self.axes, shape = _tables.pack_model(m, icols, backend.array)
        self.bc, self.bc_axes, bshape = _tables.pack_bc(ic, bands, backend.array)
        self.Q, self.B = shape[3], bshape[4]
        hot = (C.c_int32 * 4)(*[icols.index(int(i)) for i in ic._cols])
        self.model = _tables.fill(_population_cabi.IsoPopulationModelTable, self.cols, self.axes, shape, hot)
        self.bct = _tables.fill(_population_cabi.IsoPopulationBcTable, self.bc, self.bc_axes, bshape, 0)


def population_tables(ic, cols, bands, backend):
    """The packed tables, made once per (interpolator, device, columns, bands) and remade when the model or the BC table was
    rebuilt (``_chain.cached_by_generation``); ``ic.release()`` drops them."""
    gen = (ic.model_grid.interp._handles.generation, ic.bc_grid.interp._handles.generation)
    return _chain.cached_by_generation(ic, "_population_tables", (backend.device, tuple(cols), tuple(bands)), gen,
                                       lambda: PopulationTables(ic, cols, bands, backend))


def _packed_columns(ic, props):
    """(the columns asked for, the columns of the packed table: those, then what is missing of the hot four)."""
    names = list(ic.model_grid.interp.columns)
    cols = names if (isinstance(props, str) and props == "all") else list(props)
    for c in cols:
        if c not in names:
            raise ValueError("the model grid has no column %r" % (c,))
    hot = [names[int(i)] for i in ic._cols]
    packed = cols + [h for h in hot if h not in cols]
    if len(packed) > _population_cabi.MAX_COLS:
        raise ValueError("at most %d model columns per call (the hot four included), got %d" % (_population_cabi.MAX_COLS, len(packed)))
    return cols, packed


def column_names(cols, bands):
    """The reference's columns of ``generate_binary(..., all_As=True)`` in the reference's order: per component (suffix _0,
    then _1) the model columns, ``<band>_mag``, distance, AV, initial_feh, requested_age, ``A_<band>``; then per band
    ``<band>_mag``, ``A_<band>`` of the system."""
    one = list(cols) + ["%s_mag" % b for b in bands]
    for extra in ("distance", "AV", "initial_feh", "requested_age"):
        if extra not in one:                                    # (a model column of that name is overwritten in place)
            one.append(extra)
    one += ["A_%s" % b for b in bands]
    names = ["%s_%d" % (c, k) for k in (0, 1) for c in one]
    for b in bands:
        names += ["%s_mag" % b, "A_%s" % b]
    return names


class _Evaluated:
    """``matrix`` [len(columns), N] where the backend keeps its arrays, one row per column of :func:`column_names`."""

    def __init__(self, backend, columns, matrix):
        self.backend, self.columns, self.matrix = backend, columns, matrix

    def row(self, name):
        return self.matrix[self.columns.index(name)]

    def as_dict(self):
        return {c: self.matrix[r] for r, c in enumerate(self.columns)}

    def frame(self):
        import pandas as pd
        return pd.DataFrame(np.ascontiguousarray(self.backend.to_host(self.matrix).T), columns=self.columns)


def _backend_for(args, backend):
    if backend is not None:
        return backend
    for a in args:
        if dev.is_tensor(a) and a.is_cuda:
            return _DeviceBackend(a.device.index)
    return _DeviceBackend(dev.current_device())


def _evaluate(ic, mass_A, mass_B, age, feh, distance, AV, bands, props, accurate, eeps, backend):
    if getattr(ic, "eep_replaces", None) == "mass":             # as the reference's IsochroneInterpolator.generate
        ic = ic.track
    if getattr(ic, "eep_replaces", None) != "age":
        raise NotImplementedError("populations need the evolution-track parametrisation")
    bands = _tables.check_bands(ic, bands, _population_cabi.MAX_BANDS)
    cols, packed = _packed_columns(ic, props)
    if accurate not in (False, True, "exact"):
        raise ValueError("accurate is False, True or 'exact'")
    given = () if eeps is None else tuple(eeps)
    if eeps is not None and len(given) != 2:
        raise ValueError("eeps is the pair (eep_A, eep_B)")
    bk = _backend_for((mass_A, mass_B, age, feh, distance, AV) + given, backend)
    xs = bk.broadcast((mass_A, mass_B, age, feh, distance, AV) + given)
    mA, mB, age, feh, dist, av = xs[:6]
    N = int(mA.shape[0])
    if eeps is None:                                            # one estimate for both components
        e = bk.eep(ic, bk.cat([mA, mB]), bk.cat([age, age]), bk.cat([feh, feh]), bool(accurate))
        eA, eB = e[:N], e[N:]
    else:
        eA, eB = xs[6], xs[7]
    # the track grid's axes are (feh, mass, eep)
    coords = bk.stack([feh, mA, eA, feh, mB, eB])
    tb = population_tables(ic, packed, bands, bk)
    Q, B = tb.Q, tb.B
    o_cols, o_mag, o_A = bk.empty(2, Q, N), bk.empty(2, B, N), bk.empty(2, B, N)
    o_sys = bk.empty(2, B, N)                                   # system magnitudes, then system extinctions
    if N:
        out = _population_cabi.IsoPopulationOut(bk.ptr(o_cols), bk.ptr(o_mag), bk.ptr(o_A), bk.ptr(o_sys[0]), bk.ptr(o_sys[1]))
        bk.call(tb, coords, dist, av, N, 2, out)
    names = column_names(cols, bands)
    extra = {"distance": dist, "AV": av, "initial_feh": feh, "requested_age": age}
    parts = []
    for c in (0, 1):
        model = o_cols[c, :len(cols)]
        own = [k for k in extra if k not in cols]
        if len(own) < 4:                                        # a model column of that name: the reference overwrites it
            model = bk.stack([extra[k] if k in extra else model[j] for j, k in enumerate(cols)])
        parts += [model, o_mag[c]]
        if own:
            parts.append(bk.stack([extra[k] for k in own]))
        parts.append(o_A[c])
    parts.append(bk.stack([o_sys[0], o_sys[1]], axis=1).reshape(2 * B, N))
    matrix = bk.cat(parts)
    assert matrix.shape[0] == len(names)
    return _Evaluated(bk, names, matrix)


def evaluate_binaries(ic, mass_A, mass_B, age, feh, distance=10.0, AV=0.0, bands=None, props="all", accurate=False,
                      eeps=None, _backend=None):
    """The columns of the reference's ``generate_binary(mass_A, mass_B, age, feh, distance=, AV=, all_As=True)`` for a batch
    of coeval pairs, as a dict of CUDA tensors keyed by the reference's column names (:func:`column_names`), without a host
    copy: the EEPs from ``ic.get_eep`` (``accurate=True`` or ``"exact"``: ``ic.solve_eep``; or ``eeps=(eep_A, eep_B)`` as
    given), then one ``iso_population_eval`` launch on the current stream.  Inputs are host arrays or CUDA tensors,
    broadcast against each other; ``mass_B = 0`` is an absent companion.  An isochrone-parametrised ``ic`` delegates to
    ``ic.track``."""
    return _evaluate(ic, mass_A, mass_B, age, feh, distance, AV, bands, props, accurate, eeps, _backend).as_dict()


# ---- the reference's distributions, every draw from a numpy.random.Generator --------------------------------------------------

def _sample(dist, n, rng):
    """``n`` draws of a prior of ours (``sample(n, rng)``) or a frozen scipy distribution (``rvs(n, random_state=rng)``)."""
    if hasattr(dist, "sample"):
        return np.asarray(dist.sample(n, rng), dtype=np.float64)
    return np.asarray(dist.rvs(n, random_state=rng), dtype=np.float64)


class StarFormationHistory:
    """Star-formation history: ``dist`` is a scipy distribution of stellar ages in Gyr, a normalised dM/dT (default:
    uniform from 0 to 10 Gyr)."""

    def __init__(self, dist=None):
        if dist is None:
            from scipy.stats import uniform
            dist = uniform(0, 10)
        self.dist = dist

    def sample_ages(self, N, rng=None):
        """``N`` ages as log10(years)."""
        rng = np.random.default_rng() if rng is None else rng
        with np.errstate(divide="ignore"):
            return np.log10(1e9 * np.asarray(self.dist.rvs(N, random_state=rng), dtype=np.float64))


class StarFormationHistoryGrid(StarFormationHistory):
    """A star-formation history in arbitrary time bins: ``t_grid`` (Gyr) drawn with the weights ``sfh_grid``."""

    def __init__(self, t_grid, sfh_grid):
        self.t_grid = np.asarray(t_grid, dtype=np.float64)
        self.sfh_grid = np.asarray(sfh_grid, dtype=np.float64)

    def sample_ages(self, N, rng=None):
        rng = np.random.default_rng() if rng is None else rng
        cdf = self.sfh_grid.cumsum() / self.sfh_grid.sum()
        i_bin = np.minimum(np.digitize(rng.random(N), cdf), self.t_grid.size - 1)
        return np.log10(1e9 * self.t_grid[i_bin])


class BinaryDistribution:
    """Primaries from ``imf``, a companion with probability ``fB`` whose mass ratio follows ``mass_ratio_distribution``
    (default: a power law of index ``gamma`` on [0.2, 1]); a single star has a secondary mass of 0."""

    def __init__(self, imf, fB=0.4, gamma=0.3, mass_ratio_distribution=None):
        self.imf, self.fB, self.gamma = imf, fB, gamma
        if mass_ratio_distribution is None:
            mass_ratio_distribution = PowerLawPrior(self.gamma, bounds=(0.2, 1))
        self.mass_ratio_distribution = mass_ratio_distribution

    def sample(self, N, rng=None):
        rng = np.random.default_rng() if rng is None else rng
        primary = _sample(self.imf, N, rng)
        is_binary = rng.random(N) < self.fB
        q = _sample(self.mass_ratio_distribution, N, rng)
        return primary, q * primary * is_binary


class StarPopulation:
    """A synthetic population over the interpolator ``ic`` (reference: populations.py:65-166)."""
    _backend = None                                             # (the CPU tests route the evaluation to the host entry)

    def __init__(self, ic, imf=None, fB=0.4, gamma=0.3, sfh=None, feh=None, mass_ratio_distribution=None, distance=10.0,
                 AV=0.0):
        self._ic = ic
        self.sfh = StarFormationHistory() if sfh is None else sfh
        self.imf = ChabrierPrior() if imf is None else imf
        self.fB, self.gamma = fB, gamma
        self.binary_distribution = BinaryDistribution(self.imf, fB=fB, gamma=gamma,
                                                      mass_ratio_distribution=mass_ratio_distribution)
        self.feh = FehPrior() if feh is None else feh
        self.distance, self.AV = distance, AV

    @property
    def ic(self):
        if isinstance(self._ic, type):
            self._ic = self._ic()
        return self._ic

    def draw(self, N, rng):
        """(primary mass, secondary mass, log10 age, [Fe/H], distance, AV) of ``N`` systems, host arrays."""
        masses, secondary = self.binary_distribution.sample(N, rng)
        ages = self.sfh.sample_ages(N, rng)
        fehs = _sample(self.feh, N, rng)
        dist = _sample(self.distance, N, rng) if hasattr(self.distance, "sample") else np.full(N, float(self.distance))
        av = _sample(self.AV, N, rng) if hasattr(self.AV, "sample") else np.full(N, float(self.AV))
        return masses, secondary, ages, fehs, dist, av

    #: the columns of the Philox plan and their streams: a column keeps its number whatever the others are
    PHILOX_COLUMNS = ("mass", "binary", "q", "age", "feh", "distance", "AV")

    def draw_plan(self):
        """The :class:`isochrones_amd.draws.DrawPlan` of ``generate(rng="philox")``: primary mass, a uniform on (0, 1) that
        is compared with ``fB``, mass ratio, log10 age, [Fe/H], distance, AV.  A distribution the device has no inverse for
        (a ``StarFormationHistoryGrid``, a scipy distribution that is not uniform) is a host column."""
        from . import draws
        from .priors import FlatPrior

        class _Ages:                                            # a star-formation history as a host column: log10 years
            def __init__(self, sfh):
                self.sfh = sfh

            def sample(self, n, rng=None):
                return self.sfh.sample_ages(n, rng)

        sfh = self.sfh
        plain = type(sfh) is StarFormationHistory and draws._is_scipy_uniform(sfh.dist)
        cols = {"mass": self.imf, "binary": FlatPrior((0.0, 1.0)), "q": self.binary_distribution.mass_ratio_distribution,
                "age": sfh.dist if plain else _Ages(sfh), "feh": self.feh,
                "distance": self.distance if hasattr(self.distance, "sample") else float(self.distance),
                "AV": self.AV if hasattr(self.AV, "sample") else float(self.AV)}
        return draws.DrawPlan(cols, streams={name: k for k, name in enumerate(self.PHILOX_COLUMNS)})

    def _philox_evaluator(self, seed, accurate, kwargs):
        """``evaluate(n, round, bad)`` of :meth:`generate` with the draws of :meth:`draw_plan`: the first round draws the
        systems 0 .. n - 1, a later one exactly the systems ``bad`` marks, through ``index``."""
        bk = kwargs["_backend"] if kwargs["_backend"] is not None else _DeviceBackend(dev.current_device())
        plan = self.draw_plan()
        device = None if isinstance(bk, _HostBackend) else bk.device
        seed = 0 if seed is None else int(seed)

        def evaluate(n, rnd, bad):
            index = None if bad is None else (bad.nonzero().reshape(-1) if dev.is_tensor(bad) else np.flatnonzero(bad))
            d = plan.draw(n, seed, round=rnd, index=index, device=device)
            secondary = d["q"] * d["mass"] * (d["binary"] < self.fB)
            return _evaluate(self.ic, d["mass"], secondary, d["age"], d["feh"], d["distance"], d["AV"], kwargs.get("bands"),
                             kwargs.get("props", "all"), accurate, None, bk)

        return evaluate

    def generate(self, N, accurate=False, exact_N=True, seed=None, as_tensors=False, rng="numpy", **kwargs):
        """``N`` systems as a DataFrame with the reference's columns in the reference's order (``as_tensors=True``: the dict
        of CUDA tensors instead).  The draws come from ``numpy.random.default_rng(seed)``.  ``exact_N=True`` redraws the
        systems whose primary fell off the model grid (``mass_0`` NaN) and evaluates them again, a smaller batch each round,
        at most ``MAX_REDRAW_ROUNDS`` times; ``exact_N=False`` drops them.  Other keywords (``bands=``, ``props=``) go to
        :func:`evaluate_binaries`.  ``rng="philox"`` draws where the systems are evaluated (:meth:`draw_plan`, ``seed=None``
        is 0): system j is then the same whatever ``N``, and ``exact_N`` redraws exactly the systems off the grid."""
        N = int(N)
        if rng not in ("numpy", "philox"):
            raise ValueError("rng is 'numpy' or 'philox'")
        kwargs.setdefault("_backend", self._backend)
        unknown = set(kwargs) - {"bands", "props", "_backend"}
        if unknown:
            raise TypeError("generate() got unexpected keywords %s" % sorted(unknown))
        if rng == "philox":
            evaluate = self._philox_evaluator(seed, accurate, kwargs)
        else:
            gen = np.random.default_rng(seed)

            def evaluate(n, rnd, bad):
                return _evaluate(self.ic, *self.draw(n, gen), kwargs.get("bands"), kwargs.get("props", "all"), accurate, None,
                                 kwargs["_backend"])

        pop = evaluate(N, 0, None)
        if "mass_0" not in pop.columns:
            raise ValueError("props must include 'mass' (rows off the grid are found by mass_0)")
        bk = pop.backend
        bad = bk.isnan(pop.row("mass_0"))
        if exact_N:
            rounds = 0
            while bk.any(bad):
                if rounds == MAX_REDRAW_ROUNDS:
                    raise RuntimeError("StarPopulation.generate: %d of %d systems are still off the model grid after %d "
                                       "rounds of redrawing - the distributions do not reach the grid (exact_N=False "
                                       "returns the rows that do)" % (bk.count(bad), N, rounds))
                rounds += 1
                pop.matrix[:, bad] = evaluate(bk.count(bad), rounds, bad).matrix
                bad = bk.isnan(pop.row("mass_0"))
        elif bk.any(bad):
            pop = _Evaluated(bk, pop.columns, bk.take(pop.matrix, ~bad))
        return pop.as_dict() if as_tensors else pop.frame()


def deredden(pop):
    """The dereddened version of a population (AV = 0), the reference's column arithmetic: every ``<band>_mag`` less its
    ``A_<band>``, per component and for the system, the extinctions and AV set to 0.  ``pop``: the DataFrame or the dict of
    tensors of :meth:`StarPopulation.generate`; a new object of the same kind is returned."""
    is_frame = not isinstance(pop, dict)
    keys = list(pop.columns) if is_frame else list(pop)
    new = pop.copy() if is_frame else {k: (v.clone() if dev.is_tensor(v) else np.array(v)) for k, v in pop.items()}
    bands = [c[:-4] for c in keys if re.search(r"(\w+)_mag$", c)]

    def zero(key):
        if is_frame:
            new[key] = 0.0
        else:
            new[key] = new[key].new_zeros(new[key].shape) if dev.is_tensor(new[key]) else np.zeros_like(new[key])

    zero("AV_0")
    zero("AV_1")
    for b in bands:
        for s in ("", "_0", "_1"):
            new["%s_mag%s" % (b, s)] = new["%s_mag%s" % (b, s)] - new["A_%s%s" % (b, s)]
            zero("A_%s%s" % (b, s))
    return new
