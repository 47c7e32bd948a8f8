"""Long-double reference of iso_cluster_lnlike (include/isochrones_amd_cluster.h), written from the operation's
description (the header), not from the kernels.

It takes exactly the C ABI's inputs in the header's layout and treats those float64 values as exact.  Everything else is
evaluated in ``np.longdouble`` (64-bit significand on x86-64): the binary magnitude, ``logaddexp``, ``ln q``, the Gaussian
terms, both trapezoids and the sum over stars.  Three float64 decisions define the operation and are kept:

* the mass-ratio cut ``q < minq`` is made on the float64 quotient ``m_k / m_j``;
* each cell's ``exp(L)`` is rounded to float64 before it is summed, so float64 underflow gives the operation's zeros;
* ``n_valid`` is clamped to ``[0, ld]``.

A row's ``lnlike`` is ``-inf`` when any ``like_s == 0``, even if another star's is NaN."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
#: most stars per vectorised block of the (j, k) grid
STAR_BLOCK = 16


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def _logaddexp(a, b):
    """max + ln(exp(a - max) + exp(b - max)): -inf on one side selects the other, NaN on either side gives NaN."""
    hi = np.where(b > a, b, a)
    return hi + np.log(np.exp(a - hi) + np.exp(b - hi))


def _row(c, n, rp, val, w, nb, npr, minq):
    """like_s [N_s] (long double) of one row: c [3 + 2 nb + npr][ld] float64, n valid EEPs."""
    ns = val.shape[1]
    like = np.zeros(ns, dtype=LD)
    if n < 2:
        return like
    eep, mass, mterm = c[0, :n], c[1, :n], c[2, :n]
    flux, mag, prop_model = c[3:3 + nb, :n], c[3 + nb:3 + 2 * nb, :n], c[3 + 2 * nb:3 + 2 * nb + npr, :n]
    ln_fb, ln_1mfb, gamma, ln_cq = (LD(v) for v in rp)
    jj, kk = np.tril_indices(n)                                         # pairs (j, k <= j), row-major
    keep = ~(mass[kk] / mass[jj] < minq)                                # the cut on the float64 quotient
    lnq = np.log(mass[kk].astype(LD) / mass[jj].astype(LD))
    pair = mterm[jj].astype(LD) + ln_cq + gamma * lnq                   # [pairs]
    binary = -2.5 * np.log10(flux[:, jj].astype(LD) + flux[:, kk].astype(LD))   # [nb, pairs]
    d = np.diff(eep.astype(LD))                                         # [n - 1]
    v, wt = val.astype(LD), w.astype(LD)
    mag_l, pm = mag.astype(LD), prop_model.astype(LD)
    seg_end = np.arange(1, n)                                            # segment (k - 1, k) of the inner trapezoid
    inner_mask = seg_end[None, :] <= np.arange(n)[:, None]               # [j, k - 1]: k <= j

    def block(s0, s1):
        vs, ws = v[:, s0:s1], wt[:, s0:s1]                               # [nb + npr, S]
        S = s1 - s0
        phot = np.zeros((S, jj.size), dtype=LD)
        for b in range(nb):
            single = ln_1mfb + -0.5 * (mag_l[b][None, :] - vs[b][:, None]) ** 2 * ws[b][:, None]          # [S, n]
            lb = ln_fb + -0.5 * (binary[b][None, :] - vs[b][:, None]) ** 2 * ws[b][:, None]               # [S, pairs]
            phot = phot + _logaddexp(lb, single[:, jj])
        prop = np.zeros((S, n), dtype=LD)
        for p in range(npr):
            prop = prop + -0.5 * (vs[nb + p][:, None] - pm[p][None, :]) ** 2 * ws[nb + p][:, None]
        L = phot + pair[None, :] + prop[:, jj]
        e64 = np.where(keep[None, :], np.exp(np.where(keep[None, :], L, 0)).astype(np.float64), 0.0)
        e = np.zeros((S, n, n), dtype=LD)
        e[:, jj, kk] = e64                                               # each cell rounded to float64, then summed
        seg = 0.5 * (e[:, :, :-1] + e[:, :, 1:]) * d[None, None, :]      # [S, j, k - 1]
        inner = np.where(inner_mask[None], seg, 0).sum(axis=2)          # I_sj
        like[s0:s1] = (0.5 * (inner[:, :-1] + inner[:, 1:]) * d[None, :]).sum(axis=1)

    with np.errstate(all="ignore"):
        step = max(1, min(STAR_BLOCK, -(-ns // _threads())))
        spans = [(s, min(s + step, ns)) for s in range(0, ns, step)]
        if len(spans) == 1:
            block(*spans[0])
        else:
            with ThreadPoolExecutor(_threads()) as ex:
                list(ex.map(lambda sp: block(*sp), spans))
    return like


def lnlike(cols, n_valid, rowpar, star_val, star_w, minq, n_bands=None, n_props=0):
    """The operation of ``iso_cluster_lnlike`` on host arrays.

    cols [P][3 + 2 N_b + N_p][ld], n_valid [P], rowpar [P][4], star_val / star_w [N_b + N_p][N_s], minq.  ``n_bands``
    defaults to what the column count leaves after ``n_props``.  Returns ``(lnlike [P], ln like_s [P][N_s])``, both long
    double."""
    cols = np.asarray(cols, dtype=np.float64)
    P, ncol, ld = cols.shape
    nb = (ncol - 3 - n_props) // 2 if n_bands is None else n_bands
    assert ncol == 3 + 2 * nb + n_props, (ncol, nb, n_props)
    val, w = np.asarray(star_val, dtype=np.float64), np.asarray(star_w, dtype=np.float64)
    assert val.shape[0] == nb + n_props and w.shape == val.shape
    rowpar = np.asarray(rowpar, dtype=np.float64).reshape(P, 4)
    nv = np.asarray(n_valid).reshape(P)
    out = np.empty(P, dtype=LD)
    per_star = np.empty((P, val.shape[1]), dtype=LD)
    for r in range(P):
        n = int(min(max(int(nv[r]), 0), ld))
        like = _row(cols[r], n, rowpar[r], val, w, nb, n_props, float(minq))
        with np.errstate(divide="ignore", invalid="ignore"):
            ln = np.log(like)
        per_star[r] = ln
        out[r] = -np.inf if np.any(like == 0) else np.sum(ln)
    return out, per_star


def row_columns(eep, mass, lndm, mags, props, alpha, gamma, fB, minq, mass_lo, mass_hi, ld=None):
    """One row's ABI columns ``[3 + 2 N_b + N_p][ld]`` and ``rowpar [4]`` from its n kept EEPs: eep, mass, lndm [n], mags
    [n, N_b], props [n, N_p].  Flux, the mass term and ``rowpar`` are computed in float64 as
    ``StarClusterModel.lnlike_device`` does; entries past n are 0."""
    mags, props = np.asarray(mags, float), np.asarray(props, float)
    n, nb = mags.shape
    npr = props.shape[1]
    ld = n if ld is None else ld
    c = np.zeros((3 + 2 * nb + npr, ld))
    a1, g1 = alpha + 1.0, gamma + 1.0
    with np.errstate(all="ignore"):
        c[0, :n] = eep
        c[1, :n] = mass
        c[2, :n] = (np.log(a1 / (mass_hi ** a1 - mass_lo ** a1)) + alpha * np.log(mass)) + lndm
        c[3:3 + nb, :n] = np.power(10.0, -0.4 * mags).T
        c[3 + nb:3 + 2 * nb, :n] = mags.T
        c[3 + 2 * nb:, :n] = props.T
        rowpar = np.array([np.log(fB), np.log(1.0 - fB), gamma, np.log(g1 / (1.0 - minq ** g1))])
    return c, rowpar


def fixture_inputs(fx):
    """ABI inputs of every row of a tests/golden/cluster fixture, from the per-EEP columns the reference computed.

    Returns dict(cols [P][ncol][ld], n_valid, rowpar, star_val, star_w, minq [P], n_bands, n_props)."""
    meta = fx["meta"]
    bands, props = meta["bands"], meta["props"]
    mass_lo, mass_hi = (float(v) for v in meta["mass_bounds"])
    ld = fx["col_eep"].shape[1]
    n_valid = fx["col_n"].astype(np.int32)
    minq = fx["minq"].astype(float)
    cols, rowpar = [], []
    for r, n in enumerate(n_valid):
        alpha, gamma, fB = fx["pars"][r, 4:7]
        c, rp = row_columns(fx["col_eep"][r, :n], fx["col_mass"][r, :n], fx["col_lndm"][r, :n], fx["col_mags"][r, :n],
                            fx["col_props"][r, :n], alpha, gamma, fB, minq[r], mass_lo, mass_hi, ld)
        cols.append(c)
        rowpar.append(rp)
    val = [fx["mag_" + b] for b in bands] + [fx["prop_" + q] for q in props]
    unc = [fx["unc_" + b] for b in bands] + [fx["propunc_" + q] for q in props]
    return dict(cols=np.array(cols), n_valid=n_valid, rowpar=np.array(rowpar), star_val=np.array(val, dtype=float),
                star_w=1.0 / np.array(unc, dtype=float) ** 2, minq=minq, n_bands=len(bands), n_props=len(props))
