"""The stored-chain layer under diagnostics, derived and predictive (isochrones_amd/_chain.py) and the layout of a catalog
result row (catalog.result_blocks), as far as they need no device: the [S, W, T, D] view <-> parameter-major storage, the
tables that follow a grid's generation, and where fit_stars_gpu writes each block of a row."""
import itertools
import types

import numpy as np
import pytest

from isochrones_amd import _chain
from isochrones_amd.catalog import result_blocks, result_columns
from isochrones_amd.derived import expand_labels, fit_param_names
from isochrones_amd.predictive import result_labels


def _view(S, W, T, D):
    return np.arange(S * W * T * D, dtype=np.float64).reshape(S, W, T, D)


def test_storage_round_trip():
    chain = _view(3, 4, 5, 2)
    storage, S, W, single = _chain.as_storage(chain)
    assert (S, W, single) == (3, 4, False) and storage.shape == (5, 2, 12) and storage.flags.c_contiguous
    for s, w, t, d in itertools.product(range(3), range(4), range(5), range(2)):
        assert storage[t, d, s * 4 + w] == chain[s, w, t, d]                # row = ensemble * W + walker
    back = _chain.from_storage(storage, S, W, single)
    assert back.shape == chain.shape and np.array_equal(back, chain)
    # one ensemble: the leading axis comes off again, and only then
    one, S1, W1, single1 = _chain.as_storage(chain[1])
    assert (S1, W1, single1) == (1, 4, True) and one.shape == (5, 2, 4)
    assert np.array_equal(_chain.from_storage(one, S1, W1, single1), chain[1])
    assert _chain.as_storage(chain[:1])[3] is False and _chain.from_storage(one, 1, 4, False).shape == (1, 4, 5, 2)
    # the storage itself, with its counts: passed on as it is
    same, S2, W2, single2 = _chain.as_storage(storage, n_ens=np.int64(3), nwalkers=4)
    assert same is storage and (S2, W2, single2) == (3, 4, False) and type(S2) is int
    assert np.array_equal(_chain.from_storage(same, S2, W2, single2), chain)


def test_a_view_of_storage_is_not_copied():
    storage = np.arange(5 * 2 * 12, dtype=np.float64).reshape(5, 2, 12)
    view = _chain.from_storage(storage, 3, 4, False)                        # what sampler.chain returns
    assert np.shares_memory(view, storage) and not view.flags.c_contiguous
    again = _chain.as_storage(view)[0]
    assert np.shares_memory(again, storage) and np.array_equal(again, storage)
    assert not np.shares_memory(_chain.as_storage(np.ascontiguousarray(view))[0], storage)     # any other chain is copied
    import torch
    ts = torch.arange(5 * 2 * 12, dtype=torch.float64).reshape(5, 2, 12)
    tv = _chain.from_storage(ts, 3, 4, False)
    assert tv.shape == (3, 4, 5, 2) and _chain.as_storage(tv)[0].data_ptr() == ts.data_ptr()
    assert torch.equal(_chain.as_storage(tv.contiguous())[0], ts)


def test_as_storage_refusals():
    chain = _view(2, 4, 3, 2)
    for kw in (dict(n_ens=2), dict(nwalkers=4)):
        with pytest.raises(ValueError, match=r"give both n_ens and nwalkers \(parameter-major storage\) or neither "
                                             r"\(a \[S, W, T, D\] chain\)"):
            _chain.as_storage(chain, **kw)
    for bad in (np.zeros((4, 3)), np.zeros((1, 2, 4, 3, 2))):
        with pytest.raises(ValueError, match=r"chain must be \[S, W, T, D\] or \[W, T, D\]"):
            _chain.as_storage(bad)


def test_check_storage_on_the_host():
    from isochrones_amd import _cabi
    x = np.zeros((6, 5, 8), dtype=np.float32)
    got, nsteps, ndim = _chain.check_storage(x, 2, 4, _cabi.CHAIN_PARAM_MAJOR, "it takes", host=True)
    assert got.dtype == np.float64 and got.flags.c_contiguous and (nsteps, ndim) == (6, 5)
    assert _chain.check_storage(np.zeros((6, 8, 5)), 2, 4, _cabi.CHAIN_ROW_MAJOR, "it takes", host=True)[1:] == (6, 5)
    with pytest.raises(ValueError, match="it takes a float64 CUDA tensor$"):
        _chain.check_storage(x, 2, 4, _cabi.CHAIN_PARAM_MAJOR, "it takes")
    with pytest.raises(ValueError, match="it takes a float64 CUDA tensor or a host numpy array"):
        _chain.check_storage([[1.0]], 1, 1, _cabi.CHAIN_PARAM_MAJOR, "it takes", host=True)
    with pytest.raises(ValueError, match=r"n_ens \* nwalkers"):
        _chain.check_storage(x, 3, 4, _cabi.CHAIN_PARAM_MAJOR, "it takes", host=True)
    with pytest.raises(ValueError, match="no stored chain"):
        _chain.check_storage(np.zeros((0, 5, 8)), 2, 4, _cabi.CHAIN_PARAM_MAJOR, "it takes", host=True)


def test_cached_by_generation_remakes_on_a_new_generation_and_only_then():
    owner, made = types.SimpleNamespace(), []

    def make():
        made.append(len(made))
        return [made[-1]]
    a = _chain.cached_by_generation(owner, "_slot", ("dev", "key"), 7, make)
    assert a == [0] and _chain.cached_by_generation(owner, "_slot", ("dev", "key"), 7, make) is a and made == [0]
    b = _chain.cached_by_generation(owner, "_slot", ("dev", "other"), 7, make)               # another key: its own entry
    assert b == [1] and _chain.cached_by_generation(owner, "_slot", ("dev", "key"), 7, make) is a
    c = _chain.cached_by_generation(owner, "_slot", ("dev", "key"), 8, make)                 # the table was rebuilt
    assert c == [2] and _chain.cached_by_generation(owner, "_slot", ("dev", "key"), 8, make) is c
    assert _chain.cached_by_generation(owner, "_slot", ("dev", "other"), 7, make) is b and made == [0, 1, 2]
    assert owner._slot[("dev", "key")] == (8, c)                                            # (generation, value), as release() finds it
    _chain.cached_by_generation(owner, "_else", 0, (1, 2), make)
    assert set(owner.__dict__) == {"_slot", "_else"} and made == [0, 1, 2, 3]


_GRID = types.SimpleNamespace(param_names=("eep", "age", "feh", "distance", "AV"))


@pytest.mark.parametrize("N", (1, 2, 3))
def test_row_blocks_tile_the_row(N):
    names = fit_param_names(_GRID, N)
    D = len(names)
    assert D == N + 4
    labels2 = expand_labels(("radius", "mass_now"), N)
    for diag, labels, bands in itertools.product((False, True), ((), labels2), ((), ("V",), ("V", "J", "K"))):
        cols = result_columns(names, diag, labels, bands)
        at = result_blocks(cols, names, diag, labels, bands)
        order = sorted(at.values(), key=lambda s: s.start)
        # every column but ok is written exactly once, ok is the last
        assert [s.start for s in order] == [0] + [s.stop for s in order[:-1]] and order[-1].stop == len(cols)
        assert at["ok"] == slice(len(cols) - 1, len(cols)) and cols[-1] == "ok"
        assert all(s.step is None and s.stop > s.start for s in order)
        # in result_columns order, each block under its own names
        want = ["quantiles", "lnpost_max", "acceptance"]
        want += ["diag", "tau_max", "rhat_max", "window_ok"] if diag else []
        want += ["derived"] if labels else []
        want += ["ppc", "ppc_nbad", "mag_quantiles", "term_chi2", "map_pars"] if bands else []
        assert [k for k, _ in sorted(at.items(), key=lambda kv: kv[1].start)] == want + ["ok"]
        stats = ("median", "p16", "p84")
        assert cols[at["quantiles"]] == ["%s_%s" % (p, s) for p in names for s in stats]
        if diag:
            assert cols[at["diag"]] == ["%s_%s" % (p, s) for p in names for s in ("tau", "ess", "rhat")]
        if labels:
            assert cols[at["derived"]] == ["%s_%s" % (l, s) for l in labels for s in stats]
        if bands:
            assert [cols[at[k]] for k in ("ppc", "ppc_nbad")] == [["ppc"], ["ppc_nbad"]]
            assert cols[at["mag_quantiles"]] == ["%s_mag_%s" % (b, s) for b in bands for s in stats]
            assert cols[at["term_chi2"]] == ["chi2_%s" % t for t in bands + ("Teff", "logg", "feh", "parallax")]
            assert cols[at["map_pars"]] == ["map_%s" % p for p in names]
            assert cols[at["ppc"].start: at["ok"].start] == result_labels(bands, names)
        for k in ("lnpost_max", "acceptance", "tau_max", "rhat_max", "window_ok", "ok"):
            assert k not in at or cols[at[k]] == [k]
        # the closed form the row had when its offsets were counted by hand
        nb = len(bands)
        width = 3 * D + 3 + (3 * D + 3 if diag else 0) + 3 * len(labels) + (2 + 4 * nb + 4 + D if bands else 0)
        assert len(cols) == width
