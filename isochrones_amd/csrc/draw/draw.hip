// Random draws of synthetic populations and injection sets for gfx950: every column of every system from one or two
// counter-based uniforms through an exact inverse distribution function.  See include/isochrones_amd_draw.h for the
// definitions, DESIGN.md section 23 for the mapping and the resources.
//
// One kernel, 256-thread workgroups (four wavefronts), float64:
//   k_draw_systems   one lane per system, grid-stride over N.  The columns run in the host's order (a parent before its
//                    child); a column's record is the same in every lane, so it is read from the kernel arguments through
//                    scalar loads and its kind is a scalar branch.  The system's values stay in eight registers, written
//                    and read through chains of selects (a run-time index would move them to LDS); a column is stored
//                    as soon as it is drawn, lane-consecutive doubles.  Only the component choices (CHABRIER, FEH) and a
//                    conditional TABLE's row differ between the lanes of a wavefront.
// draw_value below is the definition: the kernel and iso_draw_systems_host compile the same lines.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_draw.h"
#include "../common/last_error.h"
#include "../common/ndtri.h"
#include "../common/philox.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int MAX_BLOCKS = ISO_DRAW_MAX_BLOCKS; // 256 compute units, 16 workgroups each, the rest by striding
constexpr int MAXC = ISO_DRAW_MAX_COLS;
constexpr int MAXK = ISO_DRAW_MAX_BINS;
constexpr double INV_ROOT2 = 0.7071067811865476;
typedef iso_draw_record Rec;
static_assert(sizeof(Rec) == 112, "record layout");
static_assert(MAXC == 8, "pick and put name eight values");

__host__ __device__ inline double phi(double z) { return 0.5 * erfc(-z * INV_ROOT2); }

// the inverse of x^alpha on a window that starts at base (POWERLAW of the header)
__host__ __device__ inline double plaw(double u, double a1, double E, double base, double hi, int mode) {
    if (mode == 1) return base * exp(u * E);
    if (mode == 2) return hi * exp(log(u) / a1);
    return base * exp(log1p(u * E) / a1);
}

// A system's eight values are eight named doubles, passed by value.  (Read through a reference or an array, the chain of
// selects below is rewritten by the compiler into one load at a selected address, and the values then live in LDS.)
struct Vals {
    double x0, x1, x2, x3, x4, x5, x6, x7;
};

// the value of column `at` among a system's eight
__host__ __device__ inline double pick(double x0, double x1, double x2, double x3, double x4, double x5, double x6, double x7,
                                       int at) {
    double v = x0;
    v = at == 1 ? x1 : v;
    v = at == 2 ? x2 : v;
    v = at == 3 ? x3 : v;
    v = at == 4 ? x4 : v;
    v = at == 5 ? x5 : v;
    v = at == 6 ? x6 : v;
    v = at == 7 ? x7 : v;
    return v;
}

// the eight with column `at` set to v
__host__ __device__ inline Vals put(double x0, double x1, double x2, double x3, double x4, double x5, double x6, double x7,
                                    int at, double v) {
    Vals r;
    r.x0 = at == 0 ? v : x0;
    r.x1 = at == 1 ? v : x1;
    r.x2 = at == 2 ? v : x2;
    r.x3 = at == 3 ? v : x3;
    r.x4 = at == 4 ? v : x4;
    r.x5 = at == 5 ? v : x5;
    r.x6 = at == 6 ? v : x6;
    r.x7 = at == 7 ? v : x7;
    return r;
}

// the bin of a parent's value on the parent's edges: e_k <= x < e_{k+1}, held to 0 .. Kp - 1
__host__ __device__ inline int bracket(const double* __restrict__ edges, int Kp, double x) {
    int k = 0;
    for (int i = 1; i < Kp; ++i) k += x >= edges[i] ? 1 : 0;
    return k;
}

// the draw of the header: record R, the uniforms u0 and u1, the parent's value xp (read by LINGAUSS and a conditional TABLE)
__host__ __device__ inline double draw_value(const Rec& R, double u0, double u1, double xp, const double* __restrict__ tables) {
    const double lo = R.lo, hi = R.hi;
    double v = 0.0;
    // the kinds that end in v = mu + sg * (+-ndtri(pz)), exponentiated or not, share the one ndtri below
    bool gauss = false, flip = false, expo = false;
    double pz = 0.5, mu = 0.0, sg = 1.0;
    switch (R.kind) {
    case ISO_DRAW_FLAT: v = lo + u0 * (hi - lo); break;
    case ISO_DRAW_FLATLOG: v = log10(u0 * R.p[1] + R.p[0]); break;
    case ISO_DRAW_POWERLAW: v = plaw(u0, R.p[0], R.p[1], lo, hi, (int)R.p[2]); break;
    case ISO_DRAW_GAUSS:
    case ISO_DRAW_TRUNCGAUSS:
        gauss = true;
        mu = R.p[0];
        sg = R.p[1];
        pz = R.p[2] + u0 * R.p[3];
        flip = R.p[4] != 0.0;
        break;
    case ISO_DRAW_LOGNORMAL:
        gauss = expo = true;
        mu = R.p[0];
        sg = R.p[1];
        pz = u0;
        break;
    case ISO_DRAW_CHABRIER: {
        const double w = R.p[0];
        if (u0 < w) {
            gauss = expo = true;
            mu = R.p[1];
            sg = R.p[2];
            pz = R.p[3] + (u0 / w) * R.p[4];
            flip = R.p[5] != 0.0;
        } else {
            v = plaw((u0 - w) / (1.0 - w), R.p[6], R.p[7], R.p[8], hi, (int)R.p[9]);
        }
        break;
    }
    case ISO_DRAW_FEH: {
        const bool local = R.p[0] != 0.0;
        const int k = u0 < R.p[1] ? 0 : (u0 < R.p[2] ? 1 : 2);
        const bool halo = k == (local ? 2 : 1);
        const int flips = (int)R.p[9];
        gauss = true;
        mu = halo ? -1.5 : (local ? (k == 0 ? 0.016 : -0.15) : -0.3);
        sg = halo ? 0.4 : (local ? (k == 0 ? 0.15 : 0.22) : 0.3);
        const double fa = k == 0 ? R.p[3] : (k == 1 ? R.p[5] : R.p[7]);
        const double df = k == 0 ? R.p[4] : (k == 1 ? R.p[6] : R.p[8]);
        pz = fa + u1 * df;
        flip = ((flips >> k) & 1) != 0;
        break;
    }
    case ISO_DRAW_LINGAUSS: {
        gauss = true;
        mu = R.p[0] + R.p[4] * (xp - R.p[5]);
        sg = R.p[1];
        double a = (lo - mu) * R.p[3], b = (hi - mu) * R.p[3];
        flip = a > 0;
        if (flip) {                             // take the mass in the lower tail: no 1 - 1
            const double t = a;
            a = -b;
            b = -t;
        }
        const double fa = phi(a), df = phi(b) - fa;
        // where the window's mass underflows at the sample, z = +inf: after the unflip and the clamp the bound next to the mean
        pz = df > 0.0 ? fa + u0 * df : (df != df ? df : 1.0);
        break;
    }
    case ISO_DRAW_TABLE: {
        const int K = (int)R.p[1], Kp = (int)R.p[2];
        const double* __restrict__ e = tables + (int64_t)R.p[0];
        const int row = Kp > 0 ? bracket(tables + (int64_t)R.p[3], Kp, xp) : 0;
        const double* __restrict__ cum = e + (K + 1) + (int64_t)row * (K + 1);
        int k = 0;
        for (int i = 1; i < K; ++i) k += u0 >= cum[i] ? 1 : 0;
        const double c0 = cum[k], c1 = cum[k + 1], e0 = e[k], e1 = e[k + 1];
        v = e0 + (u0 - c0) / (c1 - c0) * (e1 - e0);
        break;
    }
    case ISO_DRAW_CONSTANT: v = R.p[0]; break;
    }
    if (gauss) {
        const double z = ndtri(pz);
        v = mu + sg * (flip ? -z : z);
        if (expo) v = exp(v);
    }
    return v < lo ? lo : (v > hi ? hi : v);
}

__host__ __device__ inline void uniforms(uint64_t seed, uint64_t j, int32_t stream, int32_t round, double& u0, double& u1) {
    uint32_t w[4];
    philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), (uint32_t)stream | ((uint32_t)round << 8), (uint32_t)ISO_DRAW_PHILOX_TAG,
                  (uint32_t)seed, (uint32_t)(seed >> 32), w);
    u0 = philox_uniform53(w[0], w[1]);
    u1 = philox_uniform53(w[2], w[3]);
}

// column `at` of system j of the header: drawn, and set among the system's eight
__host__ __device__ inline double draw_column(const Rec& R, int at, uint64_t seed, uint64_t j, int32_t round,
                                              const double* __restrict__ tables, double& x0, double& x1, double& x2,
                                              double& x3, double& x4, double& x5, double& x6, double& x7) {
    double u0, u1;
    uniforms(seed, j, R.stream, round, u0, u1);
    const double v = draw_value(R, u0, u1, pick(x0, x1, x2, x3, x4, x5, x6, x7, R.parent), tables);
    const Vals n = put(x0, x1, x2, x3, x4, x5, x6, x7, at, v);
    x0 = n.x0;
    x1 = n.x1;
    x2 = n.x2;
    x3 = n.x3;
    x4 = n.x4;
    x5 = n.x5;
    x6 = n.x6;
    x7 = n.x7;
    return v;
}

struct KArgs {
    Rec rec[MAXC];                              // in evaluation order
    int32_t slot[MAXC];                         // the column of the call rec[c] is
    const double* tables;
    const int64_t* index;
    double* x;
    uint64_t seed, first;
    int64_t N;
    int32_t C, round;
};

__global__ void __launch_bounds__(BLOCK, 4) k_draw_systems(const KArgs A) {
    const int64_t N = A.N;
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < N; i += step) {
        const uint64_t j = A.index ? (uint64_t)A.index[i] : A.first + (uint64_t)i;
        double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, x4 = 0.0, x5 = 0.0, x6 = 0.0, x7 = 0.0;
#pragma unroll 1
        for (int c = 0; c < A.C; ++c) {
            const int at = A.slot[c];
            A.x[(int64_t)at * N + i] = draw_column(A.rec[c], at, A.seed, j, A.round, A.tables, x0, x1, x2, x3, x4, x5, x6, x7);
        }
    }
}

bool takes_parent(int kind) { return kind == ISO_DRAW_LINGAUSS || kind == ISO_DRAW_TABLE; }

// what is wrong with record R of a C-column call, or null; the tables are not read here (they may be device memory)
const char* record_error(const Rec& R, int q, int C, int64_t n_tables) {
    if (R.kind < ISO_DRAW_FLAT || R.kind > ISO_DRAW_CONSTANT) return "unknown kind";
    if (R.stream < 0 || R.stream > 255) return "stream must be 0 to 255";
    if (R.lo != R.lo || R.hi != R.hi || R.lo > R.hi) return "bounds must be lo <= hi";
    if (R.kind == ISO_DRAW_LINGAUSS || (R.kind == ISO_DRAW_TABLE && R.p[2] != 0.0)) {
        if (R.parent < 0 || R.parent >= C || R.parent == q) return "parent must be another column of the call";
    } else if (R.parent != -1) {
        return "parent must be -1 for a column that follows none";
    }
    switch (R.kind) {
    case ISO_DRAW_FLAT:
        if (!(R.hi - R.lo < HUGE_VAL)) return "FLAT needs finite bounds";
        break;
    case ISO_DRAW_FLATLOG:
        if (!(R.p[0] >= 0.0 && R.p[1] > 0.0 && R.p[1] < HUGE_VAL)) return "FLATLOG needs 0 <= 10^lo < 10^hi, finite";
        break;
    case ISO_DRAW_POWERLAW: {
        const double m = R.p[2];
        if (!(m == 0.0 || m == 1.0 || m == 2.0)) return "POWERLAW mode must be 0, 1 or 2";
        if (!(R.lo >= 0.0 && R.hi > R.lo && R.hi < HUGE_VAL)) return "POWERLAW needs 0 <= lo < hi, finite";
        if (m == 2.0 ? !(R.lo == 0.0 && R.p[0] > 0.0) : !(R.lo > 0.0)) return "POWERLAW from lo = 0 needs alpha > -1 and mode 2";
        if (m == 0.0 && !(R.p[0] != 0.0 && R.p[1] >= -1.0 && R.p[1] < HUGE_VAL)) return "POWERLAW mode 0 needs alpha + 1 != 0 and a finite E >= -1";
        break;
    }
    case ISO_DRAW_GAUSS:
    case ISO_DRAW_TRUNCGAUSS:
        if (!(R.p[1] > 0.0)) return "sigma must be positive";
        if (!(R.p[3] > 0.0 && R.p[2] >= 0.0 && R.p[2] + R.p[3] <= 1.0 + 1e-12)) return "a Gaussian window without mass";
        break;
    case ISO_DRAW_LOGNORMAL:
        if (!(R.p[1] > 0.0)) return "sigma must be positive";
        break;
    case ISO_DRAW_CHABRIER:
        if (!(R.p[0] >= 0.0 && R.p[0] <= 1.0)) return "CHABRIER: the lower piece's share must be 0 to 1";
        if (R.p[0] > 0.0 && !(R.p[2] > 0.0 && R.p[4] > 0.0 && R.p[3] >= 0.0)) return "CHABRIER: a lower piece without mass";
        if (R.p[0] < 1.0 && !((R.p[9] == 0.0 || R.p[9] == 1.0) && R.p[8] > 0.0)) return "CHABRIER: bad power-law piece";
        break;
    case ISO_DRAW_FEH:
        if (!(R.p[1] >= 0.0 && R.p[1] <= R.p[2] && R.p[2] <= 1.0)) return "FEH: the cumulated weights must ascend to 1";
        if (!(R.p[9] >= 0.0 && R.p[9] <= 7.0)) return "FEH: bad flip bits";
        for (int k = 0; k < 3; ++k) {
            const double w = k == 0 ? R.p[1] : (k == 1 ? R.p[2] - R.p[1] : 1.0 - R.p[2]);
            if (w > 0.0 && !(R.p[4 + 2 * k] > 0.0 && R.p[3 + 2 * k] >= 0.0)) return "a Gaussian window without mass";
        }
        break;
    case ISO_DRAW_LINGAUSS:
        if (!(R.p[1] > 0.0 && R.p[3] > 0.0)) return "sigma must be positive";
        if (!(R.hi - R.lo < HUGE_VAL)) return "LINGAUSS needs finite bounds";
        break;
    case ISO_DRAW_TABLE: {
        const double off = R.p[0], K = R.p[1], Kp = R.p[2], poff = R.p[3];
        if (!(K >= 1.0 && K <= MAXK && K == (double)(int)K)) return "a TABLE has 1 to 64 bins";
        if (!(Kp >= 0.0 && Kp <= MAXK && Kp == (double)(int)Kp)) return "a TABLE's parent has 1 to 64 bins";
        const double rows = Kp > 0.0 ? Kp : 1.0;
        if (!(off >= 0.0 && off == floor(off) && off + (K + 1.0) * (1.0 + rows) <= (double)n_tables))
            return "a TABLE lies outside the tables buffer";
        if (Kp > 0.0 && !(poff >= 0.0 && poff == floor(poff) && poff + Kp + 1.0 <= (double)n_tables))
            return "a TABLE's parent edges lie outside the tables buffer";
        break;
    }
    }
    return nullptr;
}

// the checks both entries make; fills K's records in evaluation order
int check(const char* who, const Rec* records, int32_t C, const int32_t* order, const double* tables, int64_t n_tables,
          int32_t round, int64_t first, int64_t N, const double* x, KArgs& K) {
    const char* why = nullptr;
    if (!records || (N > 0 && !x)) why = "null pointer";
    else if (C < 1 || C > MAXC) why = "C must be 1 to 8 columns";
    else if (N < 0) why = "N must not be negative";
    else if (round < 0 || round >= (1 << 24)) why = "round must be 0 to 2^24 - 1";
    else if (first < 0) why = "first must not be negative";
    else if (n_tables < 0 || n_tables > ((int64_t)1 << 40) || (n_tables > 0 && !tables)) why = "bad tables buffer";
    if (why) return fail(ISO_DRAW_ERR_INVALID, who, why);
    bool done[MAXC] = {false, false, false, false, false, false, false, false};
    for (int c = 0; c < C; ++c) {
        const int q = order ? order[c] : c;
        if (q < 0 || q >= C || done[q]) return fail(ISO_DRAW_ERR_INVALID, who, "order must be a permutation of the columns");
        const Rec& R = records[q];
        if ((why = record_error(R, q, C, n_tables))) return fail(ISO_DRAW_ERR_INVALID, who, why);
        if (R.parent >= 0 && !done[R.parent])
            return fail(ISO_DRAW_ERR_INVALID, who, "a column comes before its parent in the order (a cycle has no order)");
        done[q] = true;
        K.rec[c] = R;
        if (R.parent < 0) K.rec[c].parent = 0;  // pick() reads a register; the value is not used
        K.slot[c] = q;
    }
    for (int c = C; c < MAXC; ++c) {
        K.rec[c] = K.rec[0];
        K.slot[c] = 0;
    }
    K.C = C;
    K.round = round;
    return 0;
}

// a TABLE's numbers, which only the host entry can look at
const char* table_error(const Rec& R, const double* tables) {
    const int K = (int)R.p[1], Kp = (int)R.p[2], rows = Kp > 0 ? Kp : 1;
    const double* e = tables + (int64_t)R.p[0];
    for (int k = 0; k < K; ++k)
        if (!(e[k] < e[k + 1]) || !(e[k + 1] - e[k] < HUGE_VAL)) return "a TABLE's edges must ascend strictly";
    for (int r = 0; r < rows; ++r) {
        const double* cum = e + (K + 1) + (int64_t)r * (K + 1);
        if (cum[0] != 0.0 || cum[K] != 1.0) return "a TABLE's cumulative masses run from 0 to 1";
        for (int k = 0; k < K; ++k)
            if (!(cum[k] <= cum[k + 1])) return "a TABLE's cumulative masses must not descend";
    }
    if (Kp > 0) {
        const double* pe = tables + (int64_t)R.p[3];
        for (int k = 0; k < Kp; ++k)
            if (!(pe[k] < pe[k + 1])) return "a TABLE's parent edges must ascend strictly";
    }
    return nullptr;
}

}  // namespace

extern "C" {

const char* iso_draw_version(void) { return "isochrones_amd draw 1"; }

const char* iso_draw_last_error(void) { return g_err; }

int iso_draw_systems(const iso_draw_record* records, int32_t C, const int32_t* order, const double* tables,
                     int64_t n_tables, uint64_t seed, int32_t round, int64_t first, const int64_t* index, int64_t N,
                     double* x, void* stream) {
    g_err[0] = 0;
    KArgs K;
    const int rc = check("iso_draw_systems", records, C, order, tables, n_tables, round, first, N, x, K);
    if (rc) return rc;
    if (N == 0) return 0;
    K.tables = tables;
    K.index = index;
    K.x = x;
    K.seed = seed;
    K.first = (uint64_t)first;
    K.N = N;
    const int64_t want = (N + BLOCK - 1) / BLOCK;
    const unsigned blocks = (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    hipLaunchKernelGGL(k_draw_systems, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, K);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_DRAW_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_draw_systems_host(const iso_draw_record* records, int32_t C, const int32_t* order, const double* tables,
                          int64_t n_tables, uint64_t seed, int32_t round, int64_t first, const int64_t* index, int64_t N,
                          double* x, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_draw_systems_host";
    KArgs K;
    const int rc = check(who, records, C, order, tables, n_tables, round, first, N, x, K);
    if (rc) return rc;
    for (int c = 0; c < C; ++c) {
        const char* why = K.rec[c].kind == ISO_DRAW_TABLE ? table_error(K.rec[c], tables) : nullptr;
        if (why) return fail(ISO_DRAW_ERR_INVALID, who, why);
    }
    for (int64_t i = 0; i < N; ++i) {
        const uint64_t j = index ? (uint64_t)index[i] : (uint64_t)first + (uint64_t)i;
        double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, x4 = 0.0, x5 = 0.0, x6 = 0.0, x7 = 0.0;
        for (int c = 0; c < C; ++c) {
            const int at = K.slot[c];
            x[(int64_t)at * N + i] = draw_column(K.rec[c], at, seed, j, round, tables, x0, x1, x2, x3, x4, x5, x6, x7);
        }
    }
    return 0;
}

int iso_draw_uniforms_host(uint64_t seed, int32_t round, const int64_t* j, int64_t n, int32_t column, double* u) {
    g_err[0] = 0;
    const char* who = "iso_draw_uniforms_host";
    if (n < 0 || (n > 0 && (!j || !u))) return fail(ISO_DRAW_ERR_INVALID, who, "null pointer or negative n");
    if (column < 0 || column > 255) return fail(ISO_DRAW_ERR_INVALID, who, "column must be 0 to 255");
    if (round < 0 || round >= (1 << 24)) return fail(ISO_DRAW_ERR_INVALID, who, "round must be 0 to 2^24 - 1");
    for (int64_t i = 0; i < n; ++i) uniforms(seed, (uint64_t)j[i], column, round, u[2 * i], u[2 * i + 1]);
    return 0;
}

}  // extern "C"
