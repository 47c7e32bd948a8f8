// ln f of a population record that may link its column to another one (include/isochrones_amd_relation.h) for host and
// device code: the kinds 1 .. 8 through family_lnf.h as they are, ISO_RELATION_LINGAUSS here.  Its truncation normaliser
// depends on the sample's parent value, so it is computed per (record, sample): TruncatedGaussian.fill's flipped
// 0.5 * (erfc - erfc), moved from the host's record packing to where the sample is.
// Internal and of internal linkage.  The source writes no fused multiply-add; it is meant for -ffp-contract=off.
#ifndef ISO_COMMON_RELATION_LNF_H
#define ISO_COMMON_RELATION_LNF_H

#include "isochrones_amd_relation.h"
#include "family_lnf.h"

namespace {

// ln f(x; R) of a LINGAUSS record given the parent's value xp
__host__ __device__ inline double lingauss_lnf(const Rec& R, double x, double xp) {
    const double mu = R.p[0] + R.p[4] * (xp - R.p[5]);
    const double z = (x - mu) * R.p[3];
    double a = (R.lo - mu) * R.p[3], b = (R.hi - mu) * R.p[3];
    if (a > 0) {                                // take the mass in the lower tail: no 1 - 1
        const double t = a;
        a = -b;
        b = -t;
    }
    const double mass = 0.5 * (erfc(-b * 0.7071067811865476) - erfc(-a * 0.7071067811865476));
    if (x < R.lo || x > R.hi) return neg_inf();
    if (!(mass > 0)) return neg_inf();
    return (-(z * z) / 2.0 + R.p[2]) - log(mass);
}

// is `parent` a column of a Q-column model that column q may follow?
__host__ __device__ inline bool parent_ok(int parent, int q, int Q) { return parent >= 0 && parent < Q && parent != q; }

// the population term of column q of a Q-column model; xs: the sample's Q values (read only where R is linked)
__host__ __device__ inline double relation_lnf(const Rec& R, double x, double lx, const double* xs, int q, int Q) {
    if (R.kind != ISO_RELATION_LINGAUSS) return lnf(R, x, lx);
    return parent_ok(R.reserved, q, Q) ? lingauss_lnf(R, x, xs[R.reserved]) : qnan();
}

}  // namespace

#endif
