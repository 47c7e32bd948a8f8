"""The one ctypes loader of the side libraries (csrc/libiso_<name>.so); each _<name>_cabi.py keeps its ABI's constants,
structures and prototypes and binds ``library_path``, ``lib`` and ``check`` from an instance of :class:`SideLibrary`.

Like :func:`isochrones_amd._cabi.lib`, torch is imported before a library is opened, so that every library binds to the HIP
runtime torch bundles.  There is no CPU fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._cabi import IsoError


class SideLibrary:
    def __init__(self, name, human, declare, label=None, path=None):
        """``name``: libiso_<name>.so and the iso_<name>_ prefix of its symbols; ``human``: what the not-found message calls
        the library; ``declare(L)``: sets restype / argtypes of everything but iso_<name>_version and iso_<name>_last_error;
        ``label``: what an error of :meth:`check` calls the ABI (default: ``name``)."""
        self.name, self.human, self.declare, self.label = name, human, declare, label or name
        self.path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libiso_%s.so" % name)
        self._lib = None

    def library_path(self) -> str:
        return self.path

    def lib(self):
        """Load (once) and return the library with argtypes set.  Raises if it is absent."""
        if self._lib is not None:
            return self._lib
        if not os.path.exists(self.path):
            raise IsoError("isochrones_amd: %s library not found at %s - build it with "
                           "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)"
                           % (self.human, self.path))
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover
            pass
        L = C.CDLL(self.path)
        for sym in ("iso_%s_version" % self.name, "iso_%s_last_error" % self.name):
            getattr(L, sym).restype = C.c_char_p
            getattr(L, sym).argtypes = []
        self.declare(L)
        self._lib = L
        return L

    def check(self, rc: int):
        if rc != 0:
            msg = getattr(self.lib(), "iso_%s_last_error" % self.name)()
            e = IsoError("isochrones_amd %s C-ABI error %d: %s" % (self.label, rc, (msg or b"").decode()))
            e.rc = rc
            raise e
