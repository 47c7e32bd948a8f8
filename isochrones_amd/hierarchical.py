"""The hierarchical (population) likelihood of a catalog from the chains its fit left on the device: which mass function,
metallicity distribution and age distribution did the stars come from?  Every star's posterior samples are reweighted
from the prior the fit used (the *interim* prior) to a population density (Hogg, Myers & Bovy 2010),

    ln L(theta) = sum_s ln (1/M) sum_m  prod_q f_q(x_q[s][m]; theta) / f0_q(x_q[s][m]),

by the HIP kernels of libiso_hier.so (``iso_hier_lnlike``; the definition is in include/isochrones_amd_hier.h) on the stored
chain where it lies: no refit, no copy to the host.  A column that is a parameter of the fit is read from the sampler's
chain; anything else (``age`` on evolution tracks, ``mass`` on isochrones) from the derived chain of
:func:`isochrones_amd.derived.derive_storage`.  On isochrones ``mass`` is the model grid's column ``mass``: the one the
model's EEP prior is stated in (``EEPPrior`` interpolates ``(mass, dm_deep)``).  The ratio is taken in the coordinates the
fit's priors are stated in - the prior of the parameter EEP replaces is ``EEPPrior.orig_prior`` of that coordinate, the
Jacobian d(orig)/d(EEP) belongs to the change of variables - so no Jacobian enters.

What the fitted population says about the individual stars (their posteriors with the population in place of the
interim prior) is :meth:`PopulationPosterior.star_posteriors` (:mod:`isochrones_amd.reweight`).

Selection effects (a magnitude-limited catalog) are corrected from an injection set: ``PopulationPosterior(...,
injections=)`` and :mod:`isochrones_amd.selection`; without one the likelihood assumes that every star of the population
could have entered the catalog.

A density that links one column to another (:class:`isochrones_amd.relations.LinearGaussian`: [Fe/H] against age) makes the
model *coupled*: its truncation normaliser differs for every (hyper row, sample), so the likelihood goes through the kernels
of libiso_relation.so (``iso_relation_lnlike``, include/isochrones_amd_relation.h), which evaluate it where the sample is.
A coupled model takes no injection set and gives no per-star posteriors yet.  A density without a shape
(:class:`isochrones_amd.binned.Histogram`: bin heights over one or two columns) makes the model *binned*: the chain is
compressed once to a table of B numbers per star and every evaluation is a contraction of that table, by the kernels of
libiso_binned.so (include/isochrones_amd_binned.h).  A mixture across columns needs no kernel (the
mean weight is linear in the density: ``logsumexp_k(ln pi_k + ell_k)`` over K rows of :meth:`PopulationPosterior.star_terms`)
and has no class here; multiple systems (N > 1) are out of scope."""
from __future__ import annotations

import copy
import ctypes as C
import math

import numpy as np

from . import _cabi, _chain, _hier_cabi as hc, device as dev
from . import priors as _p

#: device memory one slice of a derived chain may take in :class:`PopulationPosterior`
HIER_BUDGET_BYTES = 2 << 30

_LOG_ROOT_2PI = math.log(math.sqrt(2 * math.pi))
_ROOT2 = math.sqrt(2.0)


def _erfc(x):
    from scipy.special import erfc
    return erfc(x)


def records(n):
    """``n`` zeroed ``iso_hier_record`` as a numpy structured array."""
    return np.zeros(n, dtype=hc.RECORD)


def prior_record(prior):
    """The ``iso_hier_record`` (a numpy structured scalar array of shape [1]) of a device prior: ``ln f`` of the record is
    ``prior.lnpdf``."""
    if _p.is_host_prior(prior):
        raise ValueError("prior %r is evaluated on the host: the hierarchical kernel needs one of "
                         "isochrones_amd.priors.DEVICE_PRIOR_TYPES" % (prior,))
    r = records(1)
    lo, hi = (float(b) for b in prior.bounds)
    r["lo"], r["hi"] = lo, hi
    with np.errstate(all="ignore"):
        if isinstance(prior, _p.FlatPrior):
            r["kind"], r["p"][0, 0] = hc.FLAT, np.log(1.0 / (hi - lo))
        elif isinstance(prior, _p.FlatLogPrior):
            r["kind"], r["p"][0, 0] = hc.FLATLOG, np.log(_p._LN10 / (10 ** hi - 10 ** lo))
        elif isinstance(prior, _p.PowerLawPrior):
            r["kind"] = hc.POWERLAW
            r["p"][0, :2] = np.log(prior._C()), prior.alpha
        elif isinstance(prior, _p.GaussianPrior):
            r["kind"] = hc.GAUSS
            if not prior.bounded:
                r["lo"], r["hi"] = -np.inf, np.inf
            r["p"][0, :4] = (prior.mean, prior.sigma, -_LOG_ROOT_2PI - math.log(prior.sigma) - prior.lognorm,
                             1.0 / prior.sigma)
        elif isinstance(prior, _p.LogNormalPrior):
            r["kind"] = hc.LOGNORMAL
            r["p"][0, :4] = (prior.mu, prior.sigma, -_LOG_ROOT_2PI - math.log(prior.sigma) - prior.mu, 1.0 / prior.sigma)
        elif isinstance(prior, _p.ChabrierPrior):
            low, high = prior.low, prior.high
            r["kind"] = hc.CHABRIER
            r["lo"], r["hi"] = (float(b) for b in high.bounds)           # the only bounds ChabrierPrior.lnpdf tests
            r["p"][0] = (low.mu, 1.0 / low.sigma, -_LOG_ROOT_2PI - math.log(low.sigma) - low.mu - prior.lognorms[0],
                         high.alpha, np.log(high._C()) - prior.lognorms[1], prior.breakpoint)
        else:
            r["kind"] = hc.FEH
            r["p"][0, :3] = prior.halo_fraction, prior._norm, 1.0 if prior.local else 0.0
    return r


class _Family:
    """One column's population density: ``names`` of its free parameters, ``ranges`` (their flat hyper-priors) and
    ``fill(rec, theta)``, which writes the records of the rows ``theta`` [H, len(names)] into ``rec`` [H]."""
    names = ()
    ranges = ()


class _Relation(_Family):
    """A family whose density depends on the same sample's value of another column of the model, ``on``
    (:mod:`isochrones_amd.relations`).  ``PopulationModel.pack`` writes the index of that column into ``reserved`` of the
    family's records."""
    on = None


class _Binned(_Family):
    """A family that is piecewise constant on the bins ``edges`` of its column (:mod:`isochrones_amd.binned`), alone or per
    bin of another such column of the model, ``given``.  ``PopulationModel`` tells it the parent's number of bins
    (``_bind``) and reads its log heights (``lnheights``); it has no records per row."""
    edges = None
    given = None


class PowerLaw(_Family):
    """x^alpha on ``bounds`` = (lo, hi), lo > 0, with ``alpha`` free in the range ``alpha`` (its flat hyper-prior);
    alpha = -1 is normalised by 1 / ln(hi / lo)."""
    names = ("alpha",)

    def __init__(self, bounds, alpha=(-5.0, 5.0)):
        self.bounds = (float(bounds[0]), float(bounds[1]))
        if not 0 < self.bounds[0] < self.bounds[1]:
            raise ValueError("PowerLaw needs bounds 0 < lo < hi")
        self.ranges = ((float(alpha[0]), float(alpha[1])),)

    def fill(self, rec, theta):
        lo, hi = self.bounds
        a = theta[:, 0]
        a1 = a + 1.0
        span = math.log(hi / lo)
        # ln C = -ln((hi^a1 - lo^a1) / a1) = -(a1 ln lo + ln(expm1(a1 span) / a1)): no cancellation near alpha = -1
        with np.errstate(all="ignore"):
            inner = np.where(a1 == 0.0, span, np.expm1(a1 * span) / np.where(a1 == 0.0, 1.0, a1))
            lnC = -(a1 * math.log(lo) + np.log(inner))
        rec["kind"], rec["lo"], rec["hi"] = hc.POWERLAW, lo, hi
        rec["p"][:, 0], rec["p"][:, 1] = lnC, a


class TruncatedGaussian(_Family):
    """A Gaussian renormalised on ``bounds`` = (lo, hi), with ``mean`` and ``sigma`` free in the ranges ``mean`` (default:
    the bounds) and ``sigma`` (default: (hi - lo) / 1000 to hi - lo)."""
    names = ("mean", "sigma")

    def __init__(self, bounds, mean=None, sigma=None):
        self.bounds = lo, hi = (float(bounds[0]), float(bounds[1]))
        if not (lo < hi and np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("TruncatedGaussian needs finite bounds lo < hi")
        mean = (lo, hi) if mean is None else mean
        sigma = ((hi - lo) / 1000.0, hi - lo) if sigma is None else sigma
        if not sigma[0] > 0:
            raise ValueError("the range of sigma must start above 0")
        self.ranges = ((float(mean[0]), float(mean[1])), (float(sigma[0]), float(sigma[1])))

    def fill(self, rec, theta):
        lo, hi = self.bounds
        mu, sg = theta[:, 0], theta[:, 1]
        with np.errstate(all="ignore"):
            a, b = (lo - mu) / sg, (hi - mu) / sg
            flip = a > 0                                            # take the mass in the lower tail: no 1 - 1
            a, b = np.where(flip, -b, a), np.where(flip, -a, b)
            mass = 0.5 * (_erfc(-b / _ROOT2) - _erfc(-a / _ROOT2))
            c = -_LOG_ROOT_2PI - np.log(sg) - np.log(mass)
        rec["kind"], rec["lo"], rec["hi"] = hc.TRUNCGAUSS, lo, hi
        rec["p"][:, 0], rec["p"][:, 1], rec["p"][:, 2], rec["p"][:, 3] = mu, sg, c, 1.0 / sg


class Fixed(_Family):
    """Any device prior as a population density without a free parameter."""

    def __init__(self, prior):
        self.prior = prior
        self._rec = prior_record(prior)

    def fill(self, rec, theta):
        rec[:] = self._rec[0]


class PopulationModel:
    """``PopulationModel(mass=PowerLaw((0.1, 10)), feh=TruncatedGaussian((-4, 0.5)))``: one family per value column, at
    most four; the density of a star's columns is their product.  A family of :mod:`isochrones_amd.relations`
    (``feh=LinearGaussian(on="age", ...)``) is conditional on another column of the model; such links may form chains but
    no cycle."""

    def __init__(self, **families):
        if not 1 <= len(families) <= hc.MAX_COLS:
            raise ValueError("a population model has 1 to %d columns (the kernel's limit)" % hc.MAX_COLS)
        for col, fam in families.items():
            if not isinstance(fam, _Family):
                raise TypeError("the family of %r must be a PowerLaw, TruncatedGaussian or Fixed (got %r)" % (col, fam))
        self.columns = tuple(families)
        self.families = tuple(families.values())
        #: per column the index of the column it is linked to, or -1
        self.parents = tuple(self._parent(col, fam) for col, fam in families.items())
        for q, col in enumerate(self.columns):
            seen, k = {q}, self.parents[q]
            while k >= 0:
                if k in seen:
                    raise ValueError("the links of the population model form a cycle through %r" % (self.columns[k],))
                seen.add(k)
                k = self.parents[k]
        self._bind_bins()
        self.param_names = tuple("%s.%s" % (c, n) for c, f in zip(self.columns, self.families) for n in f.names)
        self.ranges = np.array([r for f in self.families for r in f.ranges], dtype=float).reshape(-1, 2)

    def _parent(self, col, fam):
        if not isinstance(fam, _Relation):
            return -1
        if fam.on == col:
            raise ValueError("the family of %r is linked to its own column" % (col,))
        if fam.on not in self.columns:
            raise ValueError("the family of %r is linked to %r, which is no column of the model (%s)"
                             % (col, fam.on, ", ".join(self.columns)))
        return self.columns.index(fam.on)

    def _bind_bins(self):
        """The binned columns: their links checked, the grid's axes (a parent before its child), the cells counted."""
        from . import _binned_cabi as bc
        cols = self.columns
        # a model's own copies: binding names the logits after the parent's bins, and an instance may serve two models
        fams = self.families = tuple(copy.copy(f) if isinstance(f, _Binned) else f for f in self.families)
        self.binned_cols = tuple(q for q, f in enumerate(fams) if isinstance(f, _Binned))
        if len(self.binned_cols) > bc.MAX_AXES:
            raise ValueError("a population model has at most %d binned columns (got %s)"
                             % (bc.MAX_AXES, ", ".join(cols[q] for q in self.binned_cols)))
        self.axes = self.binned_cols
        for q in self.binned_cols:
            fam = fams[q]
            if fam.given is None:
                fam._bind(None)
                continue
            if fam.given == cols[q]:
                raise ValueError("the histogram of %r is given its own column" % (cols[q],))
            if fam.given not in cols:
                raise ValueError("the histogram of %r is given %r, which is no column of the model (%s)"
                                 % (cols[q], fam.given, ", ".join(cols)))
            parent = cols.index(fam.given)
            if not isinstance(fams[parent], _Binned):
                raise ValueError("the histogram of %r is given %r, which is no Histogram column" % (cols[q], fam.given))
            if fams[parent].given is not None:
                raise ValueError("the histograms of %r and %r are given each other" % (cols[q], fam.given))
            fam._bind(len(fams[parent].edges) - 1)
            self.axes = (parent, q)
        self.n_cells = int(np.prod([len(fams[q].edges) - 1 for q in self.axes])) if self.axes else 0
        if self.n_cells > bc.MAX_CELLS:
            raise ValueError("the grid of %s has %d cells, more than %d (the kernel's limit)"
                             % (" x ".join(cols[q] for q in self.axes), self.n_cells, bc.MAX_CELLS))

    @property
    def binned(self):
        """True if a family is a histogram: the likelihood then goes through libiso_binned.so."""
        return bool(self.binned_cols)

    def unbinnable(self):
        """The columns of a binned model whose family has free parameters but is no histogram: such a weight does not
        compress."""
        return tuple(c for c, f in zip(self.columns, self.families) if not isinstance(f, _Binned) and len(f.names))

    def bin_grid(self):
        """The grid of a binned model: ``axes`` (column indices, a parent before its child), ``edges`` (one array per
        axis), ``n_cells``, ``frozen_cols`` and ``frozen`` ([Q] records, zero at the axes)."""
        if not self.binned:
            raise ValueError("the population model has no Histogram column")
        bad = self.unbinnable()
        if bad:
            raise ValueError("a binned population model takes no family with free parameters next to its histograms (%s): "
                             "such a weight does not compress" % ", ".join(bad))
        frozen = np.zeros(len(self.families), dtype=hc.RECORD)
        frozen_cols = tuple(q for q in range(len(self.families)) if q not in self.binned_cols)
        for q in frozen_cols:
            one = np.zeros(1, dtype=hc.RECORD)
            self.families[q].fill(one, np.empty((1, 0)))
            frozen[q] = one[0]
        return dict(axes=self.axes, edges=[self.families[q].edges for q in self.axes], n_cells=self.n_cells,
                    frozen_cols=frozen_cols, frozen=frozen)

    def cell_table(self, theta):
        """``theta`` [H, P] -> :meth:`bin_grid`'s dict and ``lnh`` [H, B]: the log density of every cell of the grid (cell
        ``b = k0 * n_bins[1] + k1``) under every row."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError("theta must be [H, %d] (%s)" % (self.n_params, ", ".join(self.param_names)))
        grid = self.bin_grid()
        H = theta.shape[0]
        start = np.concatenate([[0], np.cumsum([len(f.names) for f in self.families])])
        lnh = np.zeros((H,) + tuple(len(e) - 1 for e in grid["edges"]))
        for a, q in enumerate(self.axes):
            fam = self.families[q]
            lh = fam.lnheights(theta[:, start[q]:start[q + 1]])           # [H, parent bins or 1, K]
            if len(self.axes) == 1:
                lnh = lnh + lh[:, 0, :]
            elif a == 0:
                lnh = lnh + lh[:, 0, :, None]
            else:
                lnh = lnh + (lh if fam.given is not None else lh[:, :1, :])
        return dict(grid, lnh=np.ascontiguousarray(lnh.reshape(H, -1)))

    @property
    def n_params(self):
        return len(self.param_names)

    @property
    def coupled(self):
        """True if a family is linked to another column: the likelihood then goes through libiso_relation.so."""
        return any(p >= 0 for p in self.parents)

    def pack(self, theta):
        """``theta`` [H, P] -> records [H, Q] (``_hier_cabi.RECORD``), whole columns at a time."""
        if self.binned:
            raise ValueError("a binned population model has no record per row and column: its rows are cell_table(theta)")
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError("theta must be [H, %d] (%s)" % (self.n_params, ", ".join(self.param_names)))
        out = np.zeros((theta.shape[0], len(self.families)), dtype=hc.RECORD)
        k = 0
        for q, fam in enumerate(self.families):
            col = np.zeros(theta.shape[0], dtype=hc.RECORD)
            fam.fill(col, theta[:, k:k + len(fam.names)])
            if self.parents[q] >= 0:
                col["reserved"] = self.parents[q]
            out[:, q] = col
            k += len(fam.names)
        return out

    def draw_plan(self, theta):
        """The :class:`isochrones_amd.draws.DrawPlan` of the model at one row ``theta`` [P] of its hyper-parameters: a column
        per family, a LinearGaussian after the column it follows, a Histogram as a table of its bin masses (the cell
        densities of :meth:`cell_table` times the bin widths; ``given=``: one row of masses per bin of the parent)."""
        from . import draws
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
        if theta.size != self.n_params:
            raise ValueError("theta must be one row of %d hyper-parameters (%s)" % (self.n_params, ", ".join(self.param_names)))
        start = np.concatenate([[0], np.cumsum([len(f.names) for f in self.families])]).astype(int)
        cols = {}
        mass = None
        if self.binned:
            ct = self.cell_table(theta[None, :])
            widths = [np.diff(e) for e in ct["edges"]]
            with np.errstate(all="ignore"):
                mass = np.exp(ct["lnh"][0]).reshape([w.size for w in widths])
            mass = mass * (widths[0] if len(widths) == 1 else widths[0][:, None] * widths[1][None, :])
        for q, (col, fam) in enumerate(zip(self.columns, self.families)):
            if not isinstance(fam, _Binned):
                cols[col] = draws.bound(fam, theta[start[q]:start[q + 1]])
            elif len(self.axes) == 1:
                cols[col] = draws.table(fam.edges, mass)
            elif q == self.axes[0]:
                cols[col] = draws.table(fam.edges, mass.sum(axis=1))
            elif fam.given is not None:
                cols[col] = draws.table(fam.edges, mass, given=fam.given, parent_edges=self.families[self.axes[0]].edges)
            else:
                cols[col] = draws.table(fam.edges, mass.sum(axis=0))
        return draws.DrawPlan(cols)

    def sample(self, theta, n, seed=0, device=None):
        """``{column: [n]}``: ``n`` systems drawn from the population density at one row ``theta`` of the hyper-parameters, by
        ``iso_draw_systems`` on ``device`` (CUDA tensors) or, with ``device=None``, by its host entry (numpy arrays): a
        synthetic catalog to check a fit against, or the columns of an injection set drawn near the fitted density."""
        return self.draw_plan(theta).draw(n, seed, device=device)

    def lnprior(self, theta):
        """The flat hyper-prior over the free ranges: -sum ln(width) inside, -inf outside; numpy [H]."""
        theta = np.asarray(theta, dtype=np.float64)
        if self.n_params == 0:
            return np.zeros(theta.shape[0])
        inside = np.all((theta >= self.ranges[:, 0]) & (theta <= self.ranges[:, 1]), axis=1)
        return np.where(inside, -np.sum(np.log(self.ranges[:, 1] - self.ranges[:, 0])), -np.inf)


def _ptr(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else dev.ptr(a)


class PopulationPosterior:
    """The posterior of a :class:`PopulationModel`'s hyper-parameters given the stored chains of a fit.

    ``source``: a :class:`~isochrones_amd.sampler.FusedEnsembleSampler` with a stored chain (a catalog's or a single
    model's), or ``(chain, names)`` - a ``[S, W, T, D]`` chain (CUDA tensor, or a host numpy array, which goes through the
    library's host entry) and its parameter names.  ``interim``: ``{column: prior}``, the priors the fit used; default: the
    priors of the model the sampler ran (for the parameter EEP replaces, ``EEPPrior.orig_prior``).  ``mask``: [S], zero for
    a star to leave out (a failed fit's borrowed walkers); default: the source's ``ok`` flags where it has them.

    ``injections``: an :class:`~isochrones_amd.selection.InjectionSet` that holds every column of ``model`` with its draw
    prior.  With it ``lnlike`` is ``L - S_unmasked * ln_alpha`` (``ln_alpha``: the log of the fraction of the row's
    population that the survey detects; -inf where that estimate is zero), and ``lnpost`` is -inf for a row whose
    ``selection_neff`` is below ``min_neff_factor * S_unmasked`` (Farr 2019).  The set is moved once to where the chain
    lies; a host chain goes through the library's host entry.  Without it nothing changes."""

    def __init__(self, source, ic, model, interim=None, mask=None, budget_bytes=None, injections=None, min_neff_factor=4.0):
        from .sampler import FusedEnsembleSampler
        self.ic, self.model = ic, model
        self.budget = HIER_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
        template = None
        if isinstance(source, FusedEnsembleSampler):
            if source._chain is None:
                raise ValueError("no stored chain")
            template = source.target.template if source.is_catalog else source.target
            if getattr(template, "N", 1) != 1:
                raise ValueError("the hierarchical likelihood is for single stars (N = 1); this fit has N = %d" % template.N)
            self.storage, self.S, self.W = source._chain.contiguous(), source.n_ensembles, source.nwalkers
            names = tuple(template.param_names)
            if mask is None:
                mask = getattr(source, "ok", None)
        else:
            try:
                chain, names = source
            except (TypeError, ValueError):
                raise ValueError("source must be a FusedEnsembleSampler or (chain [S, W, T, D], parameter names)") from None
            names = tuple(names)
            if len(chain.shape) != 4 or chain.shape[3] != len(names):
                raise ValueError("chain must be [S, W, T, D] with D = %d parameter names" % len(names))
            self.storage, self.S, self.W, _ = _chain.as_storage(chain)
        self.host = isinstance(self.storage, np.ndarray)
        self.storage, self.T, self.D = _chain.check_storage(self.storage, self.S, self.W, _cabi.CHAIN_PARAM_MAJOR,
                                                            "the hierarchical likelihood takes", host=True)
        if self.D != len(names):
            raise ValueError("the chain has %d parameters, %d names" % (self.D, len(names)))
        self.chain_names = names
        # where every column is read from
        self.chain_cols, self.derived_cols = {}, []
        have = ic.model_grid.interp.column_index if ic is not None else {}
        for col in model.columns:
            if col in names:
                self.chain_cols[col] = names.index(col)
            elif col in have:
                if self.host:
                    raise ValueError("column %r is a model-grid column: it is derived on the device, so the chain must be a "
                                     "CUDA tensor" % (col,))
                self.derived_cols.append(col)
            else:
                raise ValueError("column %r is neither a parameter of the chain (%s) nor a column of the model grid"
                                 % (col, ", ".join(names)))
        # the interim priors
        if interim is None:
            if template is None:
                raise ValueError("a chain without its sampler needs interim={column: prior the fit used}")
            interim = {}
            for col in model.columns:
                if col == "distance" and source.is_catalog:
                    raise ValueError("a catalog bounds the distance star by star (from its parallax): pass interim= with the "
                                     "distance prior to reweight from")
                if col == ic.eep_replaces:
                    interim[col] = template._priors["eep"].orig_prior
                elif col in template._priors and col != "eep":
                    interim[col] = template._priors[col]
        missing = [c for c in model.columns if c not in interim]
        if missing:
            raise ValueError("no interim prior for %s: pass interim={column: prior the fit used}" % ", ".join(missing))
        for col in model.columns:
            if _p.is_host_prior(interim[col]):
                raise ValueError("the interim prior of %r is evaluated on the host; the hierarchical kernel needs one of "
                                 "isochrones_amd.priors.DEVICE_PRIOR_TYPES" % (col,))
        self.interim = np.concatenate([prior_record(interim[c]) for c in model.columns])
        cost = self.T * self.W * 8 * max(1, len(self.derived_cols))
        self.step = min(self.S, self.budget // cost)
        if self.step < 1:
            raise ValueError("the columns of one star take %d bytes, more than budget_bytes = %d: raise the budget or thin "
                             "the chain" % (cost, self.budget))
        if mask is not None:
            mask = mask.detach().cpu().numpy() if dev.is_tensor(mask) else np.asarray(mask)
            if mask.shape != (self.S,):
                raise ValueError("mask must be [S] = [%d]" % self.S)
            mask = np.ascontiguousarray(mask != 0, dtype=np.int32)
        self.mask = mask
        self._dev = None            # device copies of the interim records and the mask; the derived chain when it is one slice
        self._sampler = self._samples = None
        self.n_unmasked = self.S if mask is None else int(mask.sum())
        self.min_neff_factor = float(min_neff_factor)
        self.injections, self.selection = injections, None
        self._tables = None         # a binned model's per-star tables, built on first use
        if model.binned:
            model.bin_grid()        # refuses a family with free parameters next to the histograms
        if injections is not None and model.coupled:
            raise ValueError("a coupled population model (%s) takes no injection set yet: the selection library evaluates "
                             "one-column families only and has no kernel for a linked one" % self._links())
        if injections is not None and model.binned:
            from .binned import BinnedSelection
            self.selection = BinnedSelection(injections, model, None if self.host else self.storage.device)
        elif injections is not None:
            from .selection import Selection
            self.selection = Selection(injections, model, None if self.host else self.storage.device)

    def _links(self):
        m = self.model
        return ", ".join("%s on %s" % (c, m.columns[p]) for c, p in zip(m.columns, m.parents) if p >= 0)

    def _uncoupled(self, what):
        if self.model.coupled:
            raise ValueError("%s needs an uncoupled population model: the reweighting library evaluates one-column "
                             "families only and has no kernel for a linked one (%s)" % (what, self._links()))

    # -- evaluation ---------------------------------------------------------------------------------------------------
    def _device_state(self):
        import torch
        if self._dev is None:
            device = self.storage.device
            st = dict(interim=torch.from_numpy(self.interim.view(np.uint8).copy()).to(device),
                      mask=None if self.mask is None else torch.from_numpy(self.mask).to(device), derived=None)
            self._dev = st
        return self._dev

    def _derived(self, s0, n):
        """The derived chain [T, len(derived_cols), n * W] of the stars [s0, s0 + n); kept when it is the whole catalog."""
        from . import derived as dv
        st = self._device_state()
        whole = s0 == 0 and n == self.S
        if whole and st["derived"] is not None:
            return st["derived"]
        out, _ = dv.derive_storage(self.storage, self.S, self.W, self.ic, tuple(self.derived_cols), ens_begin=s0, n_ens_out=n)
        if whole:
            st["derived"] = out
        return out

    def _columns(self, derived, s0, n):
        cols = (hc.IsoHierColumn * len(self.model.columns))()
        for q, col in enumerate(self.model.columns):
            if col in self.chain_cols:
                cols[q] = hc.IsoHierColumn(_ptr(self.storage).value, self.D, self.chain_cols[col], self.S, 0)
            else:
                cols[q] = hc.IsoHierColumn(_ptr(derived).value, len(self.derived_cols), self.derived_cols.index(col), n, s0)
        return cols

    def bin_tables(self):
        """``(A [B, S], A2 [B, S], mx [S], n_bad [S], n_out [S])`` of a binned model, where the chain lies: every star's
        samples compressed to the cells of the model's grid (include/isochrones_amd_binned.h).  Built on first use (with
        derived columns slice by slice under ``budget_bytes``; the derived chain is not kept) and read-only afterwards."""
        if self._tables is not None:
            return self._tables
        from . import _binned_cabi as bc
        from . import derived as dv
        grid = self.model.bin_grid()
        Q, S, B = len(self.model.columns), self.S, grid["n_cells"]
        i32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
        axes, n_bins = i32(grid["axes"]), i32([len(e) - 1 for e in grid["edges"]])
        frozen_cols = i32(grid["frozen_cols"])
        edges = np.ascontiguousarray(np.concatenate(grid["edges"]), dtype=np.float64)
        lib = bc.lib()
        if self.host:
            A, A2, mx = np.empty((B, S)), np.empty((B, S)), np.empty(S)
            n_bad, n_out = np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int32)
            interim, frozen, mask, fn, stream = self.interim, grid["frozen"], self.mask, lib.iso_binned_compress_host, None
        else:
            import torch
            device = self.storage.device
            st = self._device_state()
            f64 = dict(dtype=torch.float64, device=device)
            A, A2, mx = torch.empty(B, S, **f64), torch.empty(B, S, **f64), torch.empty(S, **f64)
            n_bad = torch.empty(S, dtype=torch.int32, device=device)
            n_out = torch.empty(S, dtype=torch.int32, device=device)
            interim, mask = st["interim"], st["mask"]
            frozen = torch.from_numpy(grid["frozen"].view(np.uint8).copy()).to(device)
            edges = torch.from_numpy(edges).to(device)
            fn, stream = lib.iso_binned_compress, dev.stream_ptr(device.index)
        for s0 in range(0, S, self.step):
            n = min(self.step, S - s0)
            derived = None
            if self.derived_cols:
                derived, _ = dv.derive_storage(self.storage, self.S, self.W, self.ic, tuple(self.derived_cols), ens_begin=s0,
                                               n_ens_out=n)
            bc.check(fn(self._columns(derived, s0, n), Q, _cabi.CHAIN_PARAM_MAJOR, self.T, S, self.W, s0, n, _ptr(interim),
                        _ptr(frozen), len(grid["frozen_cols"]), frozen_cols, len(grid["axes"]), axes, n_bins, _ptr(edges),
                        None, _ptr(mask), _ptr(A), _ptr(A2), _ptr(mx), _ptr(n_bad), _ptr(n_out), stream))
        self._tables = (A, A2, mx, n_bad, n_out)
        return self._tables

    def _evaluate_binned(self, theta, totals=False):
        """:meth:`_evaluate` for a binned model: the rows' log cell densities contracted with :meth:`bin_tables`.  With
        ``totals`` only ``L`` and ``min_ess`` are brought to where ``theta`` lies (the star terms of 1 024 rows x 10^4 stars
        are 164 MB, and the kernels that wrote them take less time than their download); the rest is None."""
        from . import _binned_cabi as bc
        as_tensor = dev.is_tensor(theta)
        th = np.atleast_2d(theta.detach().cpu().numpy() if as_tensor else np.asarray(theta, dtype=np.float64))
        lnh = self.model.cell_table(th)["lnh"]
        A, A2, mx, n_bad, _ = self.bin_tables()
        (H, B), S = lnh.shape, self.S
        lib = bc.lib()
        if self.host:
            ell, ess, L, mn = np.empty((H, S)), np.empty((H, S)), np.empty(H), np.empty(H)
            mask, fn, stream = self.mask, lib.iso_binned_lnlike_host, None
        else:
            import torch
            device = self.storage.device
            f64 = dict(dtype=torch.float64, device=device)
            ell, ess, L, mn = torch.empty(H, S, **f64), torch.empty(H, S, **f64), torch.empty(H, **f64), torch.empty(H, **f64)
            mask, lnh = self._device_state()["mask"], torch.from_numpy(lnh).to(device)
            fn, stream = lib.iso_binned_lnlike, dev.stream_ptr(device.index)
        bc.check(fn(_ptr(A), _ptr(A2), _ptr(mx), B, S, 0, S, self.T * self.W, _ptr(lnh), H, _ptr(mask), _ptr(ell), _ptr(ess),
                    _ptr(L), _ptr(mn), stream))
        out = (L, mn) if totals else (L, mn, ell, ess, n_bad)
        if as_tensor and self.host:
            import torch
            out = tuple(torch.from_numpy(o).to(theta.device) for o in out)
        elif not as_tensor and not self.host:
            out = tuple(o.cpu().numpy() for o in out)
        return out + (None, None, None) if totals else out

    def _evaluate(self, theta, totals=False):
        """``(L [H], min_ess [H], ell [H, S], ess [H, S], n_bad [S])`` of the rows ``theta`` [H, P]: CUDA tensors for a
        CUDA tensor ``theta``, numpy arrays otherwise."""
        if self.model.binned:                   # histograms: the chain compressed once, then libiso_binned.so's contraction
            return self._evaluate_binned(theta, totals)
        as_tensor = dev.is_tensor(theta)
        th = theta.detach().cpu().numpy() if as_tensor else np.asarray(theta, dtype=np.float64)
        th = np.atleast_2d(th)
        rows = self.model.pack(th)
        H, Q, S = rows.shape[0], rows.shape[1], self.S
        if self.model.coupled:                  # a linked family: the same call, answered by libiso_relation.so
            from . import _relation_cabi as rl
            lib, check = rl.lib(), rl.check
            fn_host, fn_dev = lib.iso_relation_lnlike_host, lib.iso_relation_lnlike
        else:
            lib, check = hc.lib(), hc.check
            fn_host, fn_dev = lib.iso_hier_lnlike_host, lib.iso_hier_lnlike
        if self.host:
            ell, ess = np.empty((H, S)), np.empty((H, S))
            n_bad, L, mn = np.empty(S, dtype=np.int32), np.empty(H), np.empty(H)
            interim, mask, drows, fn, stream = self.interim, self.mask, rows, fn_host, None
        else:
            import torch
            device = self.storage.device
            st = self._device_state()
            f64 = dict(dtype=torch.float64, device=device)
            ell, ess = torch.empty(H, S, **f64), torch.empty(H, S, **f64)
            n_bad, L, mn = torch.empty(S, dtype=torch.int32, device=device), torch.empty(H, **f64), torch.empty(H, **f64)
            interim, mask = st["interim"], st["mask"]
            drows = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1)).to(device)
            fn, stream = fn_dev, dev.stream_ptr(device.index)
        for s0 in range(0, S, self.step):
            n = min(self.step, S - s0)
            last = s0 + n == S
            derived = self._derived(s0, n) if self.derived_cols else None
            check(fn(self._columns(derived, s0, n), Q, _cabi.CHAIN_PARAM_MAJOR, self.T, S, self.W, s0, n, _ptr(interim),
                     _ptr(drows), H, _ptr(mask), _ptr(ell), _ptr(ess), _ptr(n_bad), _ptr(L if last else None),
                     _ptr(mn if last else None), stream))
        out = (L, mn, ell, ess, n_bad)
        if as_tensor and self.host:
            import torch
            out = tuple(torch.from_numpy(o).to(theta.device) for o in out)
        elif not as_tensor and not self.host:
            out = tuple(o.cpu().numpy() for o in out)
        return out

    def _alpha(self, theta):
        """``(ln_alpha [H], n_eff [H])`` from the injection set, like :meth:`_evaluate`'s results."""
        if self.selection is None:
            raise ValueError("this posterior has no injection set (injections=)")
        as_tensor = dev.is_tensor(theta)
        th = np.atleast_2d(theta.detach().cpu().numpy() if as_tensor else np.asarray(theta, dtype=np.float64))
        la, ne, _ = self.selection.alpha(th)
        if as_tensor and self.host:
            import torch
            la, ne = (torch.from_numpy(o).to(theta.device) for o in (la, ne))
        elif not as_tensor and not self.host:
            la, ne = (o.cpu().numpy() for o in (la, ne))
        return la, ne

    def _selected(self, theta):
        """``(L - S_unmasked * ln_alpha [H], n_eff [H])``.  A row whose estimate of alpha is zero (no detected injection
        in its support) is -inf."""
        la, ne = self._alpha(theta)
        L = self._evaluate(theta, totals=True)[0]
        if dev.is_tensor(L):
            import torch
            ll = torch.where(torch.isneginf(la), la, L - self.n_unmasked * la)
        else:
            with np.errstate(invalid="ignore"):
                ll = np.where(np.isneginf(la), -np.inf, L - self.n_unmasked * la)
        return ll, ne

    def lnlike(self, theta):
        """ln L of every row of ``theta`` [H, P]: [H]; with an injection set, corrected for the selection."""
        if self.selection is None:
            return self._evaluate(theta, totals=True)[0]
        return self._selected(theta)[0]

    def ln_alpha(self, theta):
        """The log of the detectable fraction of every row's population, from the injection set: [H]."""
        return self._alpha(theta)[0]

    def selection_neff(self, theta):
        """The effective number of injections behind every row's ``ln_alpha``: [H]."""
        return self._alpha(theta)[1]

    def min_ess(self, theta):
        """The smallest effective sample size among the stars, per row: [H].  Below a few, the row's ln L rests on one or two
        samples of some star and is not to be trusted."""
        return self._evaluate(theta, totals=True)[1]

    def star_terms(self, theta):
        """``(ell [H, S], ess [H, S], n_bad [S])``: every star's term of ln L, its effective sample size under the row, and
        how many of its samples were bad (NaN, or outside the interim prior).  NaN for a masked star."""
        return self._evaluate(theta)[2:]

    def star_posteriors(self, theta=None, columns=None, q=(0.5, 0.16, 0.84), as_tensors=False):
        """Every star's posterior once the population replaces the interim prior (:mod:`isochrones_amd.reweight`; the
        kernels of libiso_reweight.so on the chain where it lies).  ``theta`` [H, P]: rows taken as equally weighted draws
        of the hyper posterior; default: at most 64 rows spread evenly over the samples of :meth:`fit_mcmc`, which must
        have run.  ``columns``: chain parameters or model-grid columns (derived on the device), model columns or not;
        default: the chain's parameters, then the model's derived columns.  ``q``: 1 to 8 probabilities.  Returns a
        DataFrame (``as_tensors=True``: a dict of tensors where the chain lies) with one row per star: per column
        ``{col}_median, _p16, _p84`` (``_q<100 p>`` for another q), ``{col}_mean``, ``{col}_sd``, then ``ess`` (the effective
        sample size of the star's weights) and ``n_bad``.  A masked star is NaN; so are the column summaries of a star with
        no weight left (its ``ess`` is 0).  On a binned model (a Histogram) the kernels are libiso_shrink.so's, the weights
        are computed once per slice of stars whatever the number of rows, and the frame has ``n_out`` next to ``n_bad``: the
        star's good samples outside the grid of bins, which weigh nothing."""
        from . import reweight
        self._uncoupled("star_posteriors")
        return reweight.star_posteriors(self, theta, columns, q, as_tensors)

    def star_weights(self, theta=None, stars=None):
        """The weights behind :meth:`star_posteriors`, ``[n, W * T]`` with sample ``m = t * W + w``, normalised to sum 1 per
        star, for weighted plots of one's own.  ``stars``: an index, a sequence of indices or a contiguous slice; default:
        all.  On the chain's device (numpy for a host chain)."""
        from . import reweight
        self._uncoupled("star_weights")
        return reweight.star_weights(self, theta, stars)

    def star_bin_probabilities(self, theta=None):
        """The posterior probability of every star lying in each cell of a binned model's grid, ``[S, B]`` (``[S, K0, K1]``
        for two binned columns, the parent's bins first), where the chain lies: which age bin a star is in once the fitted
        histogram replaces the interim prior.  From the per-star tables alone, without reading the chain again
        (``iso_shrink_cells``).  ``theta``: as in :meth:`star_posteriors`.  A star's row sums to 1; a masked star and a star
        with no weight left are NaN.  A model without a Histogram raises ``ValueError``."""
        from . import reweight
        return reweight.bin_probabilities(self, theta)

    # -- maximum likelihood for a binned model (isochrones_amd.binfit; the kernels of libiso_binfit.so) ---------------------
    def cell_counts(self, theta, pairs=False):
        """``(N [H, B], n_live [H])`` of a binned model under the rows ``theta`` [H, P], where ``theta`` lies: the expected
        number of stars in every cell (the sum over the live stars of their posterior cell probabilities, for one row the
        star-sum of :meth:`star_bin_probabilities`) and the number of live stars (unmasked, with weight under the row).
        ``pairs=True``: ``(N, C [H, B, B], n_live)`` with ``C`` the sum of the outer products of the cell probabilities.
        From the per-star tables alone (``iso_binfit_moments``).  A model without a Histogram raises ``ValueError``."""
        from . import binfit
        return binfit.cell_counts(self, theta, pairs)

    def grad(self, theta):
        """The derivative of :meth:`lnlike` with respect to every hyper-parameter of a binned model, ``[H, P]`` where
        ``theta`` lies; with an injection set the selection term is included.  A model without a Histogram raises."""
        from . import binfit
        return binfit.grad(self, theta)

    def hessian(self, theta):
        """The second derivative of :meth:`lnlike` with respect to the hyper-parameters of a binned model, ``[H, P, P]``."""
        from . import binfit
        return binfit.hessian(self, theta)

    def maximize(self, theta0=None, max_iter=2000, tol=1e-8, errors=True):
        """The maximum-likelihood hyper-parameters of a binned model by EM on the cell masses, a
        :class:`~isochrones_amd.binfit.BinnedFit`.  ``theta0``: one row to start from; default: uniform cell masses.  Every
        step takes the expected counts of :meth:`cell_counts` and raises :meth:`lnlike`, which is evaluated after every step;
        it stops when the rise is below ``tol`` nats or after ``max_iter`` steps.  A logit that leaves its ``logits`` range is
        clipped and listed in ``on_bound``; the rise is promised only while none is.  ``errors``: the Laplace covariance of
        the logits from :meth:`hessian` and the standard deviation of every cell's mass by the delta method.  Two independent
        Histograms with an injection set, and a cell with expected stars that no detected injection covers, raise
        ``ValueError``; so does a model without a Histogram."""
        from . import binfit
        return binfit.maximize(self, theta0, max_iter, tol, errors)

    # -- bootstrap errors for a binned model (isochrones_amd.emfit; the kernels of libiso_emfit.so) -------------------------
    def em_masses(self, weights=None, g0=None, max_iter=2000, tol=1e-8):
        """A batch of weighted EM fits of a binned model's cell masses on the per-star tables, the whole iteration in one
        kernel where the chain lies (``iso_emfit_run``): numpy ``(g [R, B], objective [R], n_iter [R], status [R], n_live
        [R])``.  ``weights`` [R, S]: a weight per replicate and star, default one replicate of ones; ``g0`` [B] or [R, B]:
        the start masses, default uniform cell masses.  A replicate stops when its weighted log likelihood rises by less than
        ``tol`` or after ``max_iter`` steps (``status``: ``isochrones_amd.emfit.STATUS_NAMES``).  With an injection set ``g``
        is the distribution of the detected stars, ``h_b a_b / alpha``; a cell that no detected injection covers and that
        holds expected stars raises :meth:`maximize`'s ``ValueError``.  A model without a Histogram, or with two independent
        ones, raises ``ValueError``."""
        from . import emfit
        return emfit.em_masses(self, weights, g0, max_iter, tol)

    def bootstrap(self, theta0=None, n_boot=200, seed=0, weights="poisson", q=(0.16, 0.5, 0.84), max_iter=2000, tol=1e-8):
        """Bootstrap errors of the maximum-likelihood cell masses of a binned model, a
        :class:`~isochrones_amd.emfit.BinnedBootstrap`: ``n_boot`` fits under resampled star weights next to the unweighted
        fit (replicate 0), all in one batch of :meth:`em_masses` from ``theta0`` (default: uniform cell masses).
        ``weights``: "poisson" (Poisson(1) counts, the bootstrap of the stars), "bayesian" (exponential weights) or an
        array [R, S]; ``seed`` fixes them.  The errors hold where a cell's mass is 0, where :meth:`maximize`'s Laplace
        covariance is NaN.  ``n_boot < 2``, a model without a Histogram and two independent Histograms raise
        ``ValueError``."""
        from . import emfit
        return emfit.bootstrap(self, theta0, n_boot, seed, weights, q, max_iter, tol)

    def lnprior(self, theta):
        lp = self.model.lnprior(theta.detach().cpu().numpy() if dev.is_tensor(theta) else np.atleast_2d(theta))
        if dev.is_tensor(theta):
            import torch
            return torch.from_numpy(lp).to(theta.device)
        return lp

    def lnpost(self, theta):
        """lnprior + lnlike; a row outside the free ranges is -inf (the kernel sees it clipped to the ranges)."""
        as_tensor = dev.is_tensor(theta)
        th = np.atleast_2d(theta.detach().cpu().numpy() if as_tensor else np.asarray(theta, dtype=np.float64))
        lp = self.model.lnprior(th)
        clipped = np.clip(th, self.model.ranges[:, 0], self.model.ranges[:, 1]) if self.model.n_params else th
        if self.selection is None:
            ll = self._evaluate(clipped, totals=True)[0]
        else:
            ll, neff = self._selected(clipped)
            ll = np.where(neff < self.min_neff_factor * self.n_unmasked, -np.inf, ll)
        with np.errstate(invalid="ignore"):
            out = np.where(np.isfinite(lp), lp + ll, -np.inf)
        out = np.where(np.isnan(out), -np.inf, out)
        if as_tensor:
            import torch
            return torch.from_numpy(out).to(theta.device)
        return out

    # -- fitting ------------------------------------------------------------------------------------------------------
    def fit_mcmc(self, nwalkers=64, nburn=200, niter=200, seed=None, p0=None):
        """Affine-invariant ensemble (framework-op :class:`~isochrones_amd.sampler.EnsembleSampler`) over the
        hyper-parameters; the walkers of a half-step are the H rows of one ``iso_hier_lnlike`` call.  ``p0`` [nwalkers, P];
        default: drawn uniformly from the middle half of every free range.
        For a binned model ``maximize().theta`` is a good centre for ``p0``."""
        import torch
        from .sampler import EnsembleSampler
        P = self.model.n_params
        if P < 1:
            raise ValueError("the population model has no free parameter")
        rng = np.random.default_rng(seed)
        lo, hi = self.model.ranges[:, 0], self.model.ranges[:, 1]
        if p0 is None:
            pos = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(nwalkers, P))
            for _ in range(20):
                bad = ~np.isfinite(self.lnpost(pos))
                if not bad.any():
                    break
                pos[bad] = rng.uniform(lo, hi, size=(int(bad.sum()), P))
        else:
            pos = np.asarray(p0, dtype=float)
        device = torch.device("cpu") if self.host else self.storage.device
        sampler = EnsembleSampler(nwalkers, P, self.lnpost, seed=int(rng.integers(2 ** 62)), device=device)
        pos, prob = sampler.run_mcmc(pos, nburn, store=False)
        sampler.reset()
        sampler.run_mcmc(pos, niter, lnprob0=prob)
        self._sampler, self._samples = sampler, None
        return sampler

    @property
    def sampler(self):
        if self._sampler is None:
            raise AttributeError("fit_mcmc must be run first")
        return self._sampler

    @property
    def samples(self):
        """DataFrame of the hyper-parameters and ``lnprob``."""
        import pandas as pd
        if self._samples is None:
            chain, lnp = self.sampler.flatchain, self.sampler.flatlnprobability
            self._samples = pd.DataFrame(chain.cpu().numpy(), columns=list(self.model.param_names))
            self._samples["lnprob"] = lnp.cpu().numpy()
        return self._samples
