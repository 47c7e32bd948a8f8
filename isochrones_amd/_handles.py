"""When native state cached by the Python layer may be reused.

``Handles`` keeps one native handle per device with the key it was built for; ``PreparedCalls`` keeps, per thread, one
prepared call per argument key with the validity value it was built under.  Both rebuild when what they were built for
has changed; nothing else in the package destroys these handles or keeps thread-locals.
"""
from __future__ import annotations

import threading

from . import _cabi


class Handles:
    """Native handles, one per device, each valid for the key it was built for.  ``generation`` is bumped whenever a
    handle is destroyed: whatever holds on to one (or to something built on one) compares it.  Generations, not pointer
    values: a new handle often lands on the address of the freed one."""

    def __init__(self, destroy):
        self._destroy = destroy         # name of the C function that frees one handle
        self._by_device = {}            # device -> (key, handle)
        self.generation = 0

    def get(self, device, key, create):
        """The handle for ``device``; one built for another key is destroyed and ``create()`` makes its successor."""
        entry = self._by_device.get(device)
        if entry is not None:
            if entry[0] == key:
                return entry[1]
            del self._by_device[device]
            getattr(_cabi.lib(), self._destroy)(entry[1])
            self.generation += 1
        h = create()
        self._by_device[device] = (key, h)
        return h

    def release(self):
        """Destroy every handle."""
        entries, self._by_device = self._by_device, {}
        for _, h in entries.values():
            getattr(_cabi.lib(), self._destroy)(h)
        self.generation += 1


class PreparedCalls:
    """This thread's prepared calls - a C entry point with its handle, argument buffers and their addresses - one per
    argument key, all valid for the value ``valid`` they were built under (a generation, a tuple of them).  Per thread:
    ctypes drops the GIL inside the C call, so two threads sharing one set of buffers would overwrite each other's."""

    __slots__ = ("_tls",)

    def __init__(self):
        self._tls = threading.local()

    def get(self, key, valid, prepare):
        """The prepared call for ``key``, from ``prepare(key)`` unless one was prepared under ``valid``."""
        d = self._tls.__dict__
        slot = d.get("slot")                            # (valid, {key: prepared call})
        if slot is None or slot[0] != valid:
            slot = d["slot"] = (valid, {})
        c = slot[1].get(key)
        if c is None:
            c = slot[1][key] = prepare(key)
        return c

    def clear(self):
        """Drop this thread's prepared calls."""
        self._tls.__dict__.pop("slot", None)
