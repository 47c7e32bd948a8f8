"""The head and the tail of a launch of the fused lnpost BATCH kernels (fast/lnpost_wave.h: k_lnpost_fast, k_lnpost_wide).

What these kernels do outside the shared evaluation is theirs alone: the parameter loads issued ahead of the axis staging,
the staging four loads at a time, the `n - 1` clamp of the lanes past the end, the row index formed again for the stores,
and - in the two one-band single-star kernels - three parameters that wait out the model gather in the lane's gather slot.
Every one of them can go wrong only at a size: a lone row, a wave that is one row short / full / one row over, a
workgroup likewise, a third workgroup that holds one row.  So for n in SIZES, in both parameter layouts:

  * lnpost, lnprior and lnlike against the CPU oracle (rtol 1e-9, the exact NaN / -inf pattern) for the two one-band
    single-star kernels, the asteroseismic form, a binary, a 13-band model of the band-tiled kernel, and catalog rows
    (per-row star index) whose stars share their priors or carry their own;
  * bit for bit against the same rows answered ONE AT A TIME by the model's resident mailbox wave (k_mailbox_lnpost: the
    per-point path shares lnpost_wave's arithmetic and none of the batch kernels' code around it).

The rows (tests/test_gpu_dispatch_table.py's small tables and seeded rows) carry NaN and infinite parameters, values
beyond every table edge, and samples inside the tables that a prior rejects (A_V above a flat prior's upper bound)."""
import numpy as np
import pytest

import isochrones_amd as ia
from tests import _fixtures as fx
from tests import test_gpu_dispatch_table as dt

pytestmark = pytest.mark.gpu
RTOL = 1e-9
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
POOL = max(SIZES)


def pool_rows(rng, kind, ns, lo, hi):
    """POOL rows whose every prefix of 63 and more holds all the special rows: dt.batch_rows' rows in the order special
    values first, then wide and near-solution rows in turn."""
    x = dt.batch_rows(rng, kind, ns, lo, hi, n=POOL)
    ncol = x.shape[1]
    special = np.concatenate([np.arange(POOL - 8 * (j + 1), POOL - 8 * (j + 1) + 6) for j in range(ncol)])
    rest = np.setdiff1d(np.arange(POOL), special)
    near, wide = rest[rest < POOL // 2], rest[rest >= POOL // 2]
    k = min(near.size, wide.size)
    mixed = np.concatenate([np.column_stack([wide[:k], near[:k]]).reshape(-1), wide[k:], near[k:]])
    order = np.concatenate([special, mixed])
    assert order.size == POOL and special.size <= 63
    return x[order]


def single_rows(x, want):
    """Rows for the one-row launches: a finite result, a NaN parameter, a sample the prior rejects inside the tables, an
    infinite parameter, and a few more."""
    post, prior, like = want
    pick = [np.flatnonzero(np.isfinite(post))[0], np.flatnonzero(np.isnan(x).any(axis=1))[0],
            np.flatnonzero(np.isneginf(prior) & np.isfinite(like))[0], np.flatnonzero(np.isinf(x).any(axis=1))[0]]
    return [int(r) for r in pick] + [0, 7, 62, 100]


class Case:
    """One model on one small table: its rows, the oracle's three arrays for them (computed once), and - where the model has
    a resident mailbox wave - the same rows answered one at a time."""

    def __init__(self, name, kind, ns, bands, kernel, mailbox=None, astero=False, custom_prior=False, seed=0):
        self.name, self.kernel, self.mailbox = name, kernel, mailbox
        rng = np.random.default_rng(seed)
        self.ic, lo, hi = dt.make_ic(kind, bands)
        self.mod = dt.make_model(self.ic, kind, ns, bands, astero=astero, custom_prior=custom_prior)
        assert self.mod.kernel_path() == "fused-packed"
        self.x = pool_rows(rng, kind, ns, lo, hi)
        oic = fx.make_oracle_ic(self.ic)
        self.want = oic.lnpost(self.mod.model_desc(), np.ascontiguousarray(self.x.T), nthreads=8)
        self.one = None
        if mailbox:
            with dt.env(ISOCHRONES_AMD_MAILBOX=None), dt.traced(name) as t:
                self.one = [np.array([f(list(r)) for r in self.x]) for f in (self.mod.lnpost, self.mod.lnprior, self.mod.lnlike)]
            assert mailbox in t.names, (name, t.names)

    def close(self):
        del self.mod
        self.ic.release()


_CASES = {}
SPECS = {
    # the two kernels without scratch (parameters in the gather slot, late row index); a flat A_V prior that ends inside the table
    "track1-1band": dict(kind="track", ns=1, bands=("G",), kernel="k_lnpost_fast<0, 1, 1, false, false>", mailbox="k_mailbox_lnpost<0, 1, 1>",
                         custom_prior=True, seed=1),
    "iso1-1band": dict(kind="iso", ns=1, bands=("G",), kernel="k_lnpost_fast<1, 1, 1, false, false>", mailbox="k_mailbox_lnpost<1, 1, 1>",
                       custom_prior=True, seed=2),
    # the asteroseismic form (no mailbox wave of its own)
    "track1-1band-astero": dict(kind="track", ns=1, bands=("G",), kernel="k_lnpost_fast<0, 1, 1, false, true>", astero=True, custom_prior=True,
                                seed=3),
    # a batch kernel without the slot form: a binary with three bands
    "iso2-3bands": dict(kind="iso", ns=2, bands=tuple(ia.grids.KNOWN_BANDS[:3]), kernel="k_lnpost_fast<1, 2, 3, false, false>",
                        mailbox="k_mailbox_lnpost<1, 2, 3>", custom_prior=True, seed=4),
    # the band-tiled kernel: 13 bands, two tiles of eight
    "iso1-13bands": dict(kind="iso", ns=1, bands=tuple(dt.ALL_BANDS[:13]), kernel="k_lnpost_wide<1, 1>", custom_prior=True, seed=5),
}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name, **SPECS[name])
    return _CASES[name]


def test_rows_hold_every_kind():
    """The first 63 rows of every pool - part of every batch but the lone rows - hold NaN parameters, values outside the
    tables, and samples a prior rejects although the tables hold them (a finite likelihood behind a prior of -inf)."""
    for name in SPECS:
        c = case(name)
        post, prior, like = (w[:63] for w in c.want)
        assert np.isnan(c.x[:63]).any(axis=1).sum() >= c.x.shape[1], name
        assert np.isinf(c.x[:63]).any(axis=1).sum() >= c.x.shape[1], name
        assert np.isneginf(post).sum() >= 3 and np.isfinite(post).sum() >= 5, name
        assert np.isnan(like).sum() >= 3, name + ": no row whose likelihood is not evaluated"
        assert (np.isneginf(prior) & np.isfinite(like)).sum() >= 1, name + ": no prior-rejected row inside the tables"
        assert np.isfinite(c.want[0]).sum() > POOL // 20, name


@pytest.mark.parametrize("soa", [True, False], ids=["soa", "aos"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(SPECS))
def test_batch_against_oracle_and_one_row_path(name, n, soa):
    import torch
    c = case(name)
    groups = [np.array([r]) for r in single_rows(c.x, c.want)] if n == 1 else [np.arange(n)]
    for rows in groups:
        x = c.x[rows]
        t = torch.as_tensor(np.ascontiguousarray(x.T if soa else x), device="cuda")
        with dt.traced(name) as tr:
            got = [g.cpu().numpy() for g in c.mod.evaluate_device(t, soa=soa, parts=True)]
            only = c.mod.evaluate_device(t, soa=soa, parts=False).cpu().numpy()       # (no part arrays: the likelihood is skipped behind a rejecting prior)
        assert [k for k in tr.names if k.startswith("k_lnpost")] == [c.kernel], (name, tr.names)
        what = "%s n=%d %s" % (name, n, "soa" if soa else "aos")
        for g, w, part in zip(got, c.want, ("lnpost", "lnprior", "lnlike")):
            fx.assert_close(g, w[rows], RTOL, what="%s %s" % (what, part))
        assert np.array_equal(only, got[0], equal_nan=True), what + ": lnpost alone differs from lnpost with its parts"
        if c.one is not None:
            for g, o, part in zip(got, c.one, ("lnpost", "lnprior", "lnlike")):
                assert np.array_equal(g, o[rows], equal_nan=True), "%s %s: batch kernel and one-row mailbox path differ in bits" % (what, part)


# ---- catalog rows: every row names its star (MULTI) ------------------------------------------------------------------------
N_STARS = 6
_CATALOGS = {}


def catalog(own):
    """(posterior, rows, star of every row, the oracle's lnpost): six stars on the one-band track table whose priors are the
    catalog's (shared: the kernel reads them from the first star's block) or - built from models with an A_V prior each -
    their own."""
    if own not in _CATALOGS:
        from isochrones_amd.catalog import CatalogPosterior
        rng = np.random.default_rng(60 + own)
        ic, lo, hi = dt.make_ic("track", ("G",))
        cat, post = dt.make_catalog(ic, "track", 1, ("G",), N_STARS, 11)
        models = [cat.model(k, ic) for k in range(N_STARS)]
        if own:
            post.close()
            for k, m in enumerate(models):
                m.set_prior(AV=ia.priors.FlatPrior((0.0, 0.5 + 0.08 * k)))
            post = CatalogPosterior(ic, models)
        x = pool_rows(rng, "track", 1, lo, hi)
        sid = (np.arange(POOL) * 5 + 1) % N_STARS                      # neighbouring lanes on different stars
        oic = fx.make_oracle_ic(ic)
        want = np.empty(POOL)
        for k in range(N_STARS):
            sel = np.flatnonzero(sid == k)
            want[sel] = oic.lnpost(models[k].model_desc(), np.ascontiguousarray(x[sel].T), nthreads=8, parts=False)
        assert np.isfinite(want).sum() > POOL // 20 and np.isneginf(want[:63]).sum() >= 3
        _CATALOGS[own] = (post, x, sid.astype(np.int32), want, ic)
    return _CATALOGS[own]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("own", [False, True], ids=["shared-priors", "own-priors"])
def test_catalog_rows_against_oracle(own, n):
    import torch
    post, x, sid, want, _ = catalog(own)
    groups = [np.array([r]) for r in (0, 7, 62, 100, 101, 102)] if n == 1 else [np.arange(n)]
    for rows in groups:
        with dt.traced("catalog") as tr:
            got = post.lnpost(torch.as_tensor(x[rows], device="cuda"), torch.as_tensor(sid[rows], device="cuda")).cpu().numpy()
        assert [k for k in tr.names if k.startswith("k_lnpost")] == ["k_lnpost_fast<0, 1, 1, true, false>"], tr.names
        fx.assert_close(got, want[rows], RTOL, what="catalog %s n=%d" % ("own priors" if own else "shared priors", n))


def test_release_tables():
    """(last in the file: the cases above share their tables and models)"""
    for c in _CASES.values():
        c.close()
    _CASES.clear()
    for post, _, _, _, ic in _CATALOGS.values():
        post.close()
        ic.release()
    _CATALOGS.clear()
