"""Population densities that link one column to another: the mean of a column's Gaussian follows the same sample's value of
a parent column ([Fe/H] against age, AV against distance, radius against mass).  The truncation normaliser of such a
Gaussian differs for every (hyper row, sample), so it is evaluated by the kernels of libiso_relation.so
(include/isochrones_amd_relation.h), not packed into the record on the host; a :class:`~isochrones_amd.hierarchical.PopulationModel`
with such a family is *coupled* and :class:`~isochrones_amd.hierarchical.PopulationPosterior` sends it to that library."""
from __future__ import annotations

import math

import numpy as np

from . import _relation_cabi as rc
from .hierarchical import _Relation

_LOG_ROOT_2PI = math.log(math.sqrt(2 * math.pi))


class LinearGaussian(_Relation):
    """A Gaussian renormalised on ``bounds`` = (lo, hi) whose mean is ``intercept + slope * (x_on - pivot)``, ``x_on`` the
    same sample's value of the model's column ``on``.  ``intercept``, ``slope`` and ``sigma`` are free in the ranges given
    (their flat hyper-priors); the defaults of ``intercept`` and ``sigma`` are :class:`TruncatedGaussian`'s of ``mean`` and
    ``sigma``: the bounds, and (hi - lo) / 1000 to hi - lo.  ``pivot`` is fixed: put it near the parent's typical value, so
    that intercept and slope are not degenerate."""
    names = ("intercept", "slope", "sigma")

    def __init__(self, on, bounds, slope, intercept=None, sigma=None, pivot=0.0):
        if not isinstance(on, str):
            raise TypeError("on must be the name of another column of the model (got %r)" % (on,))
        self.on = on
        self.bounds = lo, hi = (float(bounds[0]), float(bounds[1]))
        if not (lo < hi and np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("LinearGaussian needs finite bounds lo < hi")
        intercept = (lo, hi) if intercept is None else intercept
        sigma = ((hi - lo) / 1000.0, hi - lo) if sigma is None else sigma
        if not sigma[0] > 0:
            raise ValueError("the range of sigma must start above 0")
        self.pivot = float(pivot)
        if not np.isfinite(self.pivot):
            raise ValueError("pivot must be finite")
        self.ranges = ((float(intercept[0]), float(intercept[1])), (float(slope[0]), float(slope[1])),
                       (float(sigma[0]), float(sigma[1])))

    def fill(self, rec, theta):
        """The records of the rows ``theta`` [H, 3]; ``reserved`` (the parent's index) is set by ``PopulationModel.pack``."""
        lo, hi = self.bounds
        b0, b1, sg = theta[:, 0], theta[:, 1], theta[:, 2]
        with np.errstate(all="ignore"):
            c = -_LOG_ROOT_2PI - np.log(sg)
            inv = 1.0 / sg
        rec["kind"], rec["lo"], rec["hi"] = rc.LINGAUSS, lo, hi
        rec["p"][:, 0], rec["p"][:, 1], rec["p"][:, 2], rec["p"][:, 3] = b0, sg, c, inv
        rec["p"][:, 4], rec["p"][:, 5] = b1, self.pivot
