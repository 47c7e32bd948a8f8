// ln f(x; record) of include/isochrones_amd_hier.h for host and device code: the family arithmetic of an iso_hier_record.
// This is its only home: csrc/hier/ and every library on its records (csrc/select/, csrc/reweight/, csrc/relation/,
// csrc/binned/) compile these lines, kernel and host entry, so a record's term is the same bits in all of them.
// Internal and of internal linkage.  The source writes no fused multiply-add; it is meant for -ffp-contract=off.
#ifndef ISO_COMMON_FAMILY_LNF_H
#define ISO_COMMON_FAMILY_LNF_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_hier.h"
#include "grid_cell.h"

namespace {

constexpr int MAXQ = ISO_HIER_MAX_COLS;
constexpr double LN10 = 2.302585092994046;

typedef iso_hier_record Rec;

__host__ __device__ inline double neg_inf() {
    union { uint64_t u; double d; } x;
    x.u = 0xfff0000000000000ULL;
    return x.d;
}

__host__ __device__ inline bool needs_log(int kind) {
    return kind == ISO_HIER_POWERLAW || kind == ISO_HIER_LOGNORMAL || kind == ISO_HIER_CHABRIER;
}

// FehPrior._shape
__host__ __device__ inline double feh_shape(double halo_fraction, bool local, double feh) {
    double disk;
    if (local) {
        const double u = feh - 0.016, v = feh + 0.15;
        disk = 1.0 / 2.5066282746310007 *
               (0.8 / 0.15 * exp(-0.5 * (u * u) / (0.15 * 0.15)) + 0.2 / 0.22 * exp(-0.5 * (v * v) / (0.22 * 0.22)));
    } else {
        const double u = feh + 0.3;
        disk = 0.3989422804014327 / 0.3 * exp(-0.5 * (u * u) / (0.3 * 0.3));
    }
    const double h = feh + 1.5;
    const double halo = 0.99735570100358173 * exp(-0.5 * (h * h) / (0.4 * 0.4));   // 1 / sqrt(2 pi 0.4^2)
    return halo_fraction * halo + (1 - halo_fraction) * disk;
}

// ln f(x; R) of the header; lx = ln x where needs_log(R.kind), unused otherwise
__host__ __device__ inline double lnf(const Rec& R, double x, double lx) {
    const bool out = x < R.lo || x > R.hi;
    switch (R.kind) {
    case ISO_HIER_FLAT: return out ? neg_inf() : R.p[0];
    case ISO_HIER_FLATLOG: return out ? neg_inf() : R.p[0] + x * LN10;
    case ISO_HIER_POWERLAW: return out ? neg_inf() : R.p[0] + R.p[1] * lx;
    case ISO_HIER_GAUSS:
    case ISO_HIER_TRUNCGAUSS: {
        const double z = (x - R.p[0]) * R.p[3];
        return out ? neg_inf() : -(z * z) / 2.0 + R.p[2];
    }
    case ISO_HIER_LOGNORMAL: {
        const double l = lx - R.p[0], v = l * R.p[3];
        return (R.p[2] - l) - 0.5 * (v * v);
    }
    case ISO_HIER_CHABRIER: {
        if (x < R.p[5]) {
            const double l = lx - R.p[0], v = l * R.p[1];
            return (R.p[2] - l) - 0.5 * (v * v);
        }
        return out ? neg_inf() : R.p[4] + R.p[3] * lx;
    }
    case ISO_HIER_FEH: return out ? neg_inf() : log(feh_shape(R.p[0], R.p[2] != 0.0, x) / R.p[1]);
    }
    return qnan();
}

}  // namespace

#endif
