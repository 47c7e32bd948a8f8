"""StarClusterModel.star_moments / star_posteriors on the device, on a small simulated cluster (20 stars, JHK, a narrow EEP
range): ln_like is lnlike_stars's per-star term bit for bit, numpy and CUDA inputs and any chunking give the same bits, and
star_posteriors is combine_star_moments of star_moments with the documented columns and index."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import cluster

pytestmark = pytest.mark.gpu

TRUTH = [9.0, 0.0, 500.0, 0.1, -2.5, 0.3, 0.3]
ROWS = np.array([TRUTH, [9.02, -0.03, 505.0, 0.12, -2.2, 0.35, 0.25], [8.97, 0.04, 492.0, 0.08, -2.8, 0.25, 0.4]])


def _model(**kw):
    ic = ia.synthetic_isochrone(bands=("J", "H", "K"))
    cat = ia.simulate_cluster(30, *TRUTH, bands="JHK", mass_range=(0.8, 0.9), ic=ic, seed=7)
    df = cat.df[np.isfinite(cat.df[["J_mag", "H_mag", "K_mag"]].to_numpy()).all(axis=1)].iloc[:20]
    df = df.set_axis(["star%02d" % i for i in range(len(df))], axis=0)
    # a narrow range of primaries, so that 150 EEPs hold them all with room below for the secondaries near them
    lo = int(np.floor(df["eep_pri"].min())) - 60
    hi = lo + 149
    assert df["eep_pri"].max() + 10 < hi, (df["eep_pri"].min(), df["eep_pri"].max())
    return ia.StarClusterModel(ic, df, bands=["J", "H", "K"], props=["parallax"], eep_bounds=(lo, hi), **kw)


@pytest.fixture(scope="module")
def mod():
    return _model()


@pytest.fixture(scope="module")
def result(mod):
    return mod.star_moments(ROWS)


def _bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_ln_like_is_the_likelihoods_per_star_term(mod, result):
    ln_like, moments = result
    ns = len(mod.stars)
    assert ns == 20 and mod._device_state(0)["eeps"].numel() <= 150
    assert isinstance(ln_like, np.ndarray) and ln_like.shape == (3, ns) and moments.shape == (3, ns, 11)
    total, per_star = mod.lnlike_stars(ROWS)
    assert _bits(ln_like, per_star)
    live = np.isfinite(ln_like)
    print("EEPs %s, live (row, star) %d of %d" % (mod.bounds("eep"), live.sum(), live.size))
    assert live.sum() >= 40 and np.isfinite(moments[live]).all() and np.isnan(moments[~live]).all()
    lo, hi = mod.bounds("eep")
    m = moments[live]
    assert np.all((m[:, 0] >= lo) & (m[:, 0] <= hi)) and np.all((m[:, 4] >= mod.minq) & (m[:, 4] <= 1.0 + 1e-12))
    assert np.all(m[:, 8] >= 0) and np.all(m[:, 9] >= 0) and np.all(m[:, 8] + m[:, 9] <= 1.0 + 1e-12)
    assert np.all(m[:, 6] <= m[:, 2] * (1 + 1e-12))                      # the secondary is the lighter one
    one, one_m = mod.star_moments(ROWS[1])
    assert _bits(one[0], ln_like[1]) and _bits(one_m[0], moments[1])


def test_cuda_in_cuda_out_and_chunks_give_the_same_bits(mod, result):
    import torch
    ln_like, moments = result
    t_ln, t_mom = mod.star_moments(torch.as_tensor(ROWS, device="cuda"))
    assert t_ln.is_cuda and t_mom.is_cuda and t_ln.dtype == torch.float64 and tuple(t_mom.shape) == moments.shape
    assert _bits(t_ln.cpu().numpy(), ln_like) and _bits(t_mom.cpu().numpy(), moments)
    one = _model(chunk_rows=1)
    c_ln, c_mom = one.star_moments(ROWS)
    assert _bits(c_ln, ln_like) and _bits(c_mom, moments)
    again = mod.star_moments(ROWS[::-1].copy())
    assert _bits(again[0][::-1], ln_like) and _bits(again[1][::-1], moments)


def test_star_posteriors_is_the_combination(mod, result):
    ln_like, moments = result
    frame = mod.star_posteriors(ROWS)
    want = cluster.combine_star_moments(ln_like, moments)
    assert tuple(frame.columns) == cluster.STAR_POSTERIOR_COLUMNS
    assert list(frame.index) == list(mod.stars.df.index) == ["star%02d" % i for i in range(20)]
    for k in cluster.STAR_POSTERIOR_COLUMNS:
        assert _bits(frame[k].to_numpy(), want[k]), k
    assert np.all(frame["n_rows"] + frame["n_dead"] == 3)
    with pytest.raises(ValueError):
        mod.star_posteriors()


def test_star_posteriors_thins_the_samples_of_a_fit(mod):
    import pandas as pd
    fitted = _model()
    rng = np.random.default_rng(2)
    chain = np.array(TRUTH) + np.array([0.01, 0.01, 2.0, 0.01, 0.1, 0.02, 0.02]) * rng.standard_normal((40, 7))
    samples = pd.DataFrame(chain, columns=list(fitted.param_names))
    samples["lnprob"] = 0.0
    fitted._samples = samples                                            # what a fit leaves behind
    frame = fitted.star_posteriors(max_rows=5)
    pick = np.linspace(0, 39, 5).round().astype(int)
    want = cluster.combine_star_moments(*fitted.star_moments(chain[pick]))
    assert np.all(frame["n_rows"] + frame["n_dead"] == 5)
    for k in cluster.STAR_POSTERIOR_COLUMNS:
        assert _bits(frame[k].to_numpy(), want[k]), k
