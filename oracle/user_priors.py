"""TEST INFRASTRUCTURE - priors a USER would write, built on whichever priors module they are given.

``make(pr)`` takes a priors module - the reference's ``isochrones.priors`` (oracle/make_golden.py) or
``isochrones_amd.priors`` (the tests) - and returns the same five classes on that module's base classes, so that ONE piece
of user code is evaluated by both sides: the reference normalises and evaluates it when the fixtures are generated, this
build does when they are checked.  Every class returns -inf outside its own bounds (the reference's ``BasicStarModel``
applies no bounds test of its own, this build applies the bounds in the kernel; that difference stays out of the fixtures).
"""
import math

import numpy as np


def make(pr):
    class Triangle(pr.Prior):
        """Only ``_pdf``: normalised by the base class's ``bounds`` setter, ``lnpdf`` = log of the base class's ``pdf``."""

        def __init__(self, bounds):
            super().__init__()
            self._lo, self._hi = float(bounds[0]), float(bounds[1])     # (the setter integrates _pdf before it stores)
            self._norm = 1.0
            self.bounds = (self._lo, self._hi)

        def _pdf(self, x):
            return (x - self._lo) + 0.05 * (self._hi - self._lo)

    class ForeignExp:
        """Not derived from anything: ``lnpdf`` / ``bounds`` / ``sample(n)`` (the reference's signature)."""

        def __init__(self, scale, bounds):
            self.scale, self.bounds = float(scale), (float(bounds[0]), float(bounds[1]))
            lo, hi = self.bounds
            self._z = self.scale * (math.exp(-lo / self.scale) - math.exp(-hi / self.scale))

        def lnpdf(self, x):
            lo, hi = self.bounds
            return -math.inf if (x < lo or x > hi) else -x / self.scale - math.log(self._z)

        def sample(self, n):
            lo, hi = self.bounds
            u = np.random.default_rng(5).random(n)
            a, b = math.exp(-lo / self.scale), math.exp(-hi / self.scale)
            return -self.scale * np.log(a - u * (a - b))

    class Skew(pr.GaussianPrior):
        """A device family's subclass with its own ``_lnpdf`` (the family's bounds test stays in front of it)."""

        def _lnpdf(self, x):
            z = (x - self.mean) / self.sigma
            return -0.5 * z * z - math.log(self.sigma) - self.lognorm + math.log1p(0.5 * math.tanh(z))

    class Tilt(pr.FlatPrior):
        """A device family's subclass with its own ``_pdf`` (integrates to one over the bounds)."""

        def _pdf(self, x):
            lo, hi = self.bounds
            w = hi - lo
            return (1.0 + 0.6 * ((x - lo) / w - 0.5)) / w

    class Over(pr.PowerLawPrior):
        """A device family's subclass that replaces ``lnpdf`` altogether, bounds test included."""

        def lnpdf(self, x, **kwargs):
            lo, hi = self.bounds
            if x < lo or x > hi:
                return -math.inf
            return -math.log(hi - lo) + 0.25 * math.sin(x / 40.0)

    return dict(Triangle=Triangle, ForeignExp=ForeignExp, Skew=Skew, Tilt=Tilt, Over=Over)


_made = {}


def build(pr, spec):
    """``("User", "Triangle", lo, hi)`` etc. -> an object of that class on the module ``pr``."""
    if pr not in _made:
        _made[pr] = make(pr)
    name, a = spec[1], [float(v) for v in spec[2:]]
    cls = _made[pr][name]
    if name in ("Triangle", "Tilt"):
        return cls((a[0], a[1]))
    if name == "ForeignExp":
        return cls(a[0], (a[1], a[2]))
    if name == "Skew":
        return cls(a[0], a[1], bounds=(a[2], a[3]))
    if name == "Over":
        return cls(a[0], (a[1], a[2]))
    raise ValueError(name)
