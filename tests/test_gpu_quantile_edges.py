"""iso_chain_quantiles_layout on the named cases of tests/_quantile_twin.py: every selection route of the seven kernels of
kernels/k_chain_quantiles.h (the LDS sort, the workgroup selection, the streamed refinement for more than 8 192 values, the two
generic wave kernels, the compile-time-shaped ones with and without a tail) and the hand-over between them, the capacity edges
(448 / 449 pool slots, lists of 128 / 129, a refinement pool of 2 048 / 2 049), the small and odd shapes, and the chains whose
range - or whose range's reciprocal - is no finite double.  tests/test_quantile_twin_cpu.py shows, without a GPU, that the
cases are on the routes they are named for.

Every case, through _cabi directly:
  * out equals the twin's answer as BYTES where that is finite; elsewhere the same class and sign, NaN exactly where the twin
    has NaN;
  * row-major and parameter-major storage give the same bytes, and so does a second call;
  * the kernels launched (iso_debug_trace_kernels) are the expected ones;
  * out lies between sentinel-filled margins, which stay untouched, and the chain's bytes are unchanged.

Not covered: the dispatch guard that keeps a chain whose lane offsets reach 2^32 bytes away from k_chain_quantiles_exact - it
needs a chain of tens of gigabytes, which no few-second test can hold.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import _quantile_twin as T

pytestmark = pytest.mark.gpu

MARGIN = 64
SENTINEL = -7.77e77


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(case, param_major, stream=None):
    """(out [S, D, nq] as numpy, kernel names); asserts the margins and the chain are left alone"""
    import torch
    from isochrones_amd import _cabi, device as dev
    lib, ctx = _cabi.lib(), dev.context(0)
    host = case.chain(param_major)
    chain = torch.as_tensor(host, device="cuda")
    n = case.S * case.D * case.q.size
    buf = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float64, device="cuda")
    out = buf[MARGIN:MARGIN + n]
    torch.cuda.synchronize()
    was = _cabi.trace_kernels(True)
    try:
        _cabi.check(lib.iso_chain_quantiles_layout(ctx, dev.ptr(chain), _cabi.CHAIN_PARAM_MAJOR if param_major else _cabi.CHAIN_ROW_MAJOR,
                                                   case.nsteps, case.S, case.W, case.D, case.q.ctypes.data_as(C.POINTER(C.c_double)),
                                                   int(case.q.size), dev.ptr(out), C.c_void_p(stream.cuda_stream) if stream else None))
        names = _cabi.traced_kernels()
    finally:
        _cabi.trace_kernels(bool(was))
    (stream.synchronize() if stream else torch.cuda.synchronize())
    got = buf.cpu().numpy()
    assert np.array_equal(_bytes(got[:MARGIN]), _bytes(np.full(MARGIN, SENTINEL))), (case.name, "margin before out")
    assert np.array_equal(_bytes(got[MARGIN + n:]), _bytes(np.full(MARGIN, SENTINEL))), (case.name, "margin after out")
    assert np.array_equal(_bytes(chain.cpu().numpy()), _bytes(host)), (case.name, "the chain was written to")
    return got[MARGIN:MARGIN + n].reshape(case.S, case.D, case.q.size), names


def _check(case, got, what):
    want = T.want(case.values, case.q)
    names = np.array([p.name for p in case.pairs]).reshape(case.S, case.D)
    fin = np.isfinite(want)
    bad = np.argwhere(_bytes(got)[fin] != _bytes(want)[fin])
    where = np.argwhere(fin)
    first = [(names[tuple(where[i][:2])], int(where[i][2]), got[tuple(where[i])], want[tuple(where[i])]) for i in bad[:6, 0]]
    pairs = collections.Counter(str(names[tuple(where[i][:2])]) for i in bad[:, 0])
    assert not bad.size, "%s (%s): %d of %d finite quantiles differ from the twin, per pair %r; (pair, level, got, want) %r" % (
        case.name, what, bad.shape[0], int(fin.sum()), dict(pairs), first)
    odd = ~fin & ~((np.isnan(got) & np.isnan(want)) | (got == want))
    assert not odd.any(), "%s (%s): non-finite quantiles of another class at %r: got %r, want %r" % (
        case.name, what, [(names[i, j], int(k)) for i, j, k in np.argwhere(odd)[:6]], got[odd][:6], want[odd][:6])


@pytest.mark.parametrize("name", [c.name for c in T.cases()])
def test_chain_quantiles_case(name, monkeypatch):
    import torch
    case = T.case(name)
    if case.mode:
        monkeypatch.setenv("ISOCHRONES_AMD_QUANTILES", case.mode)
    else:
        monkeypatch.delenv("ISOCHRONES_AMD_QUANTILES", raising=False)
    stream = torch.cuda.Stream() if case.stream else None
    got_pm, names = _run(case, True, stream)
    assert names == case.kernels, (case.name, names, case.kernels)
    _check(case, got_pm, "parameter-major")
    got_rm, names = _run(case, False, stream)
    assert names == case.kernels, (case.name, names, case.kernels)
    _check(case, got_rm, "row-major")
    assert np.array_equal(_bytes(got_rm), _bytes(got_pm)), (case.name, "the two layouts differ")
    again, _ = _run(case, True, stream)
    assert np.array_equal(_bytes(again), _bytes(got_pm)), (case.name, "a second call differs")

