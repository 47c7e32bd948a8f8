#!/usr/bin/env python
"""TEST INFRASTRUCTURE - regenerate tests/golden/population/binary.npz by running the reference's own
``generate_binary(..., all_As=True)`` (isochrones/models.py:580-661) on the small synthetic tables of
oracle/make_golden.py (``small_track()``: 18 columns, ``small_bc()``: 7 bands) for 200 coeval pairs.

Needs a checkout of the reference (oracle/ref_harness.py: $ISO_REFERENCE_ROOT):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_population_golden.py [out_dir]

Nothing under oracle/ is changed; the harness is used as it is, with one addition made here: the generator attaches to its
own instance of the reference's interpolator a ``get_eep`` that hands back the EEPs the generator has chosen (the
primaries' on the first call, the secondaries' on the second: ``generate_binary`` calls ``generate`` once per component).
This is data the reference reads, not a change to its arithmetic: the EEP estimate is no part of what the fixture pins,
everything after it is.

The reference's interpolator reads node i + 1 of an axis with weight 0 for a coordinate exactly on node i, the last node
included (isochrones/interp.py:296-336), where that read is past the table: compiled it multiplies whatever lies there by
zero, run as plain Python (as here) it raises IndexError.  So that the rows with AV on the last A node can be evaluated
at all, the reference is handed the BC table with one more A node behind the last (AV = 2, a copy of the last node's
values); every other row brackets the same cell with the same weights as on the table itself, and a row on AV = 1 gets
the node's value times 1 plus a finite value times 0.  The tests evaluate on the table without that node.

The draw.  Primary masses come from the cool part of the mass axis (0.35 to 1.25 Msun): the BC table ends at Teff = 8356 K
and the hot half of the axis falls off it.  One secondary in five is absent (mass 0, EEP NaN), the others have a mass
ratio in [0.35, 1].  [Fe/H] and the EEPs are uniform over their axes, AV over [0, 1], the distance over [20, 1000] pc;
``age`` is only recorded by the reference (``requested_age``).  Rows kept on purpose: 8 with AV exactly 0, 8 with AV on the
last node of the A axis, 6 with a primary off the mass axis (a NaN primary), 6 with a primary beyond the BC table (model
columns but no magnitude).  The generator asserts on what it writes: at most 40 % of the rows with a NaN system magnitude,
at least 30 % with a present secondary and finite magnitudes, at least 5 rows of each kind kept on purpose.

The fixture holds the inputs (``mass_A``, ``mass_B``, ``age``, ``feh``, ``distance``, ``AV``), the EEPs (``eep_A``,
``eep_B``), ``columns`` (the reference's DataFrame columns, in its order) and ``values`` [200, len(columns)].  It holds no
table: the tests rebuild the tables from oracle/make_golden.py.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh                    # noqa: E402,F401
from oracle import make_golden as mg                    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "population")
N = 200
SEED = 20240917


def draw(rng, ax, av_axis):
    f, m, e = ax
    mass_A = rng.uniform(0.35, 1.25, N)
    absent = rng.integers(0, 5, N) == 0
    mass_B = np.where(absent, 0.0, mass_A * rng.uniform(0.35, 1.0, N))
    feh = rng.uniform(f[0], f[-1], N)
    eep_A = rng.uniform(e[0], e[-1], N)
    eep_B = np.where(absent, np.nan, rng.uniform(e[0], e[-1], N))
    age = rng.uniform(8.0, 8.6, N)
    distance = rng.uniform(20.0, 1000.0, N)
    AV = rng.uniform(av_axis[0], av_axis[-1], N)
    AV[0:8] = 0.0
    AV[8:16] = av_axis[-1]
    mass_A[16:22] = rng.uniform(0.1, 0.25, 6)                   # below the mass axis: a NaN primary
    mass_A[22:28] = rng.uniform(6.0, 7.9, 6)                    # at their first EEPs: beyond the BC table
    eep_A[22:28] = rng.uniform(e[0], e[3], 6)
    mass_B[22:28] = np.where(mass_B[22:28] > 0, 0.9, 0.0)
    return mass_A, mass_B, age, feh, distance, AV, eep_A, eep_B


def main(out=OUT):
    g, ax, cols = mg.small_track()
    ax = tuple(np.asarray(a, dtype=float) for a in ax)
    bc = mg.small_bc()
    # one more A node behind the last, for the reference alone (see above)
    padded = (np.concatenate([bc[0], bc[0][:, :, :, -1:]], axis=3), tuple(bc[1][:3]) + (np.append(bc[1][3], 2.0),), bc[2])
    ic = rh.make_ref_ic("track", (g, ax, cols), padded, mg.limits_of("track", ax), (ax[2][0], ax[2][-1]))
    rng = np.random.default_rng(SEED)
    mass_A, mass_B, age, feh, distance, AV, eep_A, eep_B = draw(rng, ax, np.asarray(bc[1][3], dtype=float))
    chosen = [eep_A, eep_B]
    ic.get_eep = lambda mass, age, feh, **kw: chosen.pop(0)     # the generator's EEPs: primaries, then secondaries
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df = ic.generate_binary(mass_A, mass_B, age, feh, distance=distance, AV=AV, all_As=True)
    assert not chosen and len(df) == N
    columns = [str(c) for c in df.columns]
    values = np.ascontiguousarray(df.values, dtype=np.float64)
    bands = list(bc[2])
    sys_mags = values[:, [columns.index("%s_mag" % b) for b in bands]]
    sec_mags = values[:, [columns.index("%s_mag_1" % b) for b in bands]]
    nan_sys = np.isnan(sys_mags).any(axis=1)
    both = (mass_B > 0) & np.isfinite(sec_mags).all(axis=1) & np.isfinite(sys_mags).all(axis=1)
    nan_primary = np.isnan(values[:, columns.index("mass_0")])
    assert nan_sys.mean() <= 0.40, nan_sys.mean()
    assert both.mean() >= 0.30, both.mean()
    assert (mass_B == 0).sum() >= 5 and nan_primary.sum() >= 5 and (AV == 0).sum() >= 5 and (AV == bc[1][3][-1]).sum() >= 5
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "binary.npz"), mass_A=mass_A, mass_B=mass_B, age=age, feh=feh, distance=distance,
                        AV=AV, eep_A=eep_A, eep_B=eep_B, columns=np.array(columns), values=values)
    print("binary systems=%d columns=%d NaN system magnitude=%.0f%% secondary present and finite=%.0f%% absent=%d "
          "NaN primary=%d" % (N, len(columns), 100 * nan_sys.mean(), 100 * both.mean(), (mass_B == 0).sum(), nan_primary.sum()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
