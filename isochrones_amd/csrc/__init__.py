#: the names the side libraries' build scripts had as modules of this package -> their specs in libraries.py
_FORMER_BUILD_SCRIPTS = {"build_cluster": "CLUSTER", "build_nested": "NESTED", "build_solve": "SOLVE", "build_diag": "DIAG",
                         "build_derived": "DERIVED", "build_predict": "PREDICT"}


def __getattr__(name):
    """``from isochrones_amd.csrc import build_solve``, which is how the test suite of every earlier commit reaches the side
    libraries: a test module that cannot import stops the whole pytest session at collection, so those suites run on this
    tree only while the names resolve.  (On demand, so that ``python -m isochrones_amd.csrc.libraries`` does not find its
    module imported already.)"""
    if name in _FORMER_BUILD_SCRIPTS:
        from . import libraries
        return getattr(libraries, _FORMER_BUILD_SCRIPTS[name])
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
