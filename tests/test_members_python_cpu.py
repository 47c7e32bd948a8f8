"""The Python layer of the per-star cluster summaries without a GPU: combine_star_moments against a direct numpy restatement
(dead rows skipped and counted, a variance that rounds below 0, q_pair at p_pair 0), star_posteriors without a fit, and the
ctypes binding against the header."""
import os
import re

import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import _members_cabi as mc
from isochrones_amd import cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("eep_A", 0), ("mass_A", 2), ("q", 4), ("mass_B", 6))


def _restated(ln_like, moments):
    """Star by star, row by row."""
    P, ns = ln_like.shape
    out = {k: np.full(ns, np.nan) for k in cluster.STAR_POSTERIOR_COLUMNS}
    out["n_rows"], out["n_dead"] = np.zeros(ns, np.int64), np.zeros(ns, np.int64)
    for s in range(ns):
        rows = [r for r in range(P) if np.isfinite(ln_like[r, s])]
        out["n_rows"][s], out["n_dead"][s] = len(rows), P - len(rows)
        if not rows:
            continue
        mean = np.array([sum(moments[r, s, m] for r in rows) / len(rows) for m in range(11)])
        for name, i in PAIRS:
            out[name][s] = mean[i]
            out[name + "_sd"][s] = np.sqrt(max(mean[i + 1] - mean[i] * mean[i], 0.0))
        out["p_pair"][s], out["p_single"][s] = mean[8], mean[9]
        out["q_pair"][s] = mean[10] / mean[8] if mean[8] != 0 else np.nan
    return out


def _draws(P, ns, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 2.0, (P, ns, 4))
    mom = np.empty((P, ns, 11))
    for i in range(4):
        mom[:, :, 2 * i] = x[:, :, i]
        mom[:, :, 2 * i + 1] = x[:, :, i] ** 2 + rng.uniform(0.0, 0.1, (P, ns))
    mom[:, :, 8] = rng.uniform(0.0, 0.6, (P, ns))
    mom[:, :, 9] = rng.uniform(0.0, 0.4, (P, ns))
    mom[:, :, 10] = mom[:, :, 8] * rng.uniform(0.1, 1.0, (P, ns))
    return rng.normal(-5.0, 1.0, (P, ns)), mom


def test_combine_matches_a_direct_restatement():
    ln, mom = _draws(7, 5, 0)
    ln[2, 1] = -np.inf                                                  # a dead row of star 1: NaN moments, as the library gives
    mom[2, 1] = np.nan
    ln[:, 3] = -np.inf                                                  # star 3 is dead in every row
    mom[:, 3] = np.nan
    ln[4, 4] = np.nan                                                   # a NaN measurement: not finite either
    mom[4, 4] = np.nan
    got, want = cluster.combine_star_moments(ln, mom), _restated(ln, mom)
    assert tuple(got) == cluster.STAR_POSTERIOR_COLUMNS
    for k in cluster.STAR_POSTERIOR_COLUMNS:
        assert got[k].shape == (5,)
        assert np.allclose(got[k], want[k], rtol=1e-14, atol=0, equal_nan=True), k
    assert list(got["n_rows"]) == [7, 6, 7, 0, 6] and list(got["n_dead"]) == [0, 1, 0, 7, 1]
    assert got["n_rows"].dtype.kind == "i" and got["n_dead"].dtype.kind == "i"
    assert all(np.isnan(got[k][3]) for k in cluster.STAR_POSTERIOR_COLUMNS[:11])
    assert all(np.isfinite(got[k][[0, 1, 2, 4]]).all() for k in cluster.STAR_POSTERIOR_COLUMNS)
    assert ia.combine_star_moments is cluster.combine_star_moments


def test_a_variance_that_rounds_below_zero_gives_sd_zero():
    ln = np.zeros((3, 2))
    mom = np.zeros((3, 2, 11))
    x = 1.0 + 2.0 ** -30
    mom[:, :, 0::2][:, :, :4] = x
    mom[:, :, 1::2][:, :, :4] = np.nextafter(x * x, 0.0)                # E[x^2] a rounding below E[x]^2
    mom[:, :, 8] = 0.5
    got = cluster.combine_star_moments(ln, mom)
    for name, _ in PAIRS:
        assert np.all(got[name] == x) and np.all(got[name + "_sd"] == 0.0), name


def test_q_pair_is_nan_where_p_pair_is_zero():
    ln, mom = _draws(4, 3, 1)
    mom[:, 1, 8] = 0.0
    mom[:, 1, 10] = 0.0
    with np.errstate(all="raise"):                                       # and no warning on the way
        got = cluster.combine_star_moments(ln, mom)
    assert np.isnan(got["q_pair"][1]) and np.isfinite(got["q_pair"][[0, 2]]).all() and got["p_pair"][1] == 0.0
    keep = mom[:, [0, 2]]
    assert np.allclose(got["q_pair"][[0, 2]], keep[:, :, 10].mean(axis=0) / keep[:, :, 8].mean(axis=0), rtol=1e-14)


def test_shapes_are_checked():
    with pytest.raises(ValueError):
        cluster.combine_star_moments(np.zeros((3, 2)), np.zeros((3, 2, 10)))
    with pytest.raises(ValueError):
        cluster.combine_star_moments(np.zeros(3), np.zeros((3, 11)))


def test_star_posteriors_needs_rows_or_a_fit():
    import pandas as pd
    ic = ia.synthetic_isochrone(bands=("J", "H", "K"))
    df = pd.DataFrame({"J_mag": [10.0, 11.0], "J_mag_unc": [0.01, 0.01], "H_mag": [9.8, 10.7], "H_mag_unc": [0.01, 0.01],
                       "K_mag": [9.7, 10.6], "K_mag_unc": [0.01, 0.01], "parallax": [2.0, 2.0], "parallax_unc": [0.2, 0.2]})
    mod = ia.StarClusterModel(ic, df, bands=["J", "H", "K"], props=["parallax"], eep_bounds=(300, 400))
    with pytest.raises(ValueError, match="fit"):
        mod.star_posteriors()
    assert callable(mod.star_moments) and callable(mod.star_moments_device)
    assert mod._rows_per_chunk(101, work_fold=6) < mod._rows_per_chunk(101) == mod._rows_per_chunk(101, work_fold=1)
    mod.chunk_rows = 3
    assert mod._rows_per_chunk(101, work_fold=6) == 3


def test_the_binding_agrees_with_the_header():
    text = open(os.path.join(ROOT, "include", "isochrones_amd_members.h")).read()
    body = text.split("#ifndef")[1]
    assert set(re.findall(r"\b(iso_members_\w+)\s*\(", body)) == set(mc.EXPORTED_SYMBOLS)
    consts = dict(re.findall(r"#define ISO_MEMBERS_(\w+) (\S+)", body))
    assert int(consts["NMOM"]) == mc.ISO_MEMBERS_NMOM == mc.NMOM == 11 == len(mc.MOMENTS)
    assert int(consts["NINNER"]) == mc.NINNER == 6
    assert int(consts["MAX_BANDS"]) == mc.MAX_BANDS == 32 and int(consts["MAX_PROPS"]) == mc.MAX_PROPS == 8
    assert int(consts["ERR_INVALID"].strip("()")) == mc.ERR_INVALID and int(consts["ERR_HIP"].strip("()")) == mc.ERR_HIP
    from isochrones_amd import _cluster_cabi as cc
    assert (mc.MAX_BANDS, mc.MAX_PROPS) == (cc.MAX_BANDS, cc.MAX_PROPS)
    assert len(cluster.STAR_POSTERIOR_COLUMNS) == 13 and cluster.STAR_POSTERIOR_COLUMNS == (
        "eep_A", "eep_A_sd", "mass_A", "mass_A_sd", "q", "q_sd", "mass_B", "mass_B_sd", "p_pair", "p_single", "q_pair", "n_rows",
        "n_dead")
