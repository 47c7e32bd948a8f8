// Nested sampling of a catalog: one workgroup per star, the live points in LDS, one launch for the whole fit.
// (libiso_nested.so; the device code of libiso_hip.so it builds on - lnpost_wave, coop_lds, philox4x32_10, uniform53 - is
// header-only and comes in through iso_fast_kernel.h)
#pragma once
#include "../../../include/isochrones_amd_nested.h"
#include "../iso_fast_kernel.h"

// -------------------------------------------------------------------------------------------
// The algorithm is nested_sample_batched (isochrones_amd/nested.py) per star; DESIGN.md "Nested sampling of a catalog" is
// the text both this kernel and its numpy twin (tests/_nested_twin.py) implement.  In short:
//   * the prior is flat on the star's box (bound_lo / bound_hi of its block), a point is u in the unit cube and
//     theta = fma(hi - lo, u, lo); loglike = lnpost, non-finite = zero likelihood;
//   * every pass of the main loop is one CHUNK of BLOCK draws, one per lane, evaluated by lnpost_wave.  Philox4x32-10,
//     key = seed, counter = (8 chunk + call, global star index low word, lane | high word << 16, 0x4E).  The chunk index
//     runs on through the whole fit;
//   * FILL: uniform draws until nlive finite ones are held (taken in draw order), prior_fraction = finite / tried over
//     whole chunks; the list is then sorted by rank counting (ascending in logl, ties by age);
//   * MACRO-STEP: the K lowest (the head of the sorted list) are retired with shrinkage 1 / (nlive - j); stop test;
//     bounding ellipsoid of the survivors; chunks of draws uniform in it (Box-Muller direction, radius u^(1/D), outside
//     the cube = not evaluated) kept when logl > thr[K - 1], in draw order, until K are held; merged into the other
//     buffer by rank counting / bisection;
//   * FINISH: the survivors retired without replacement, the last one taking the remaining volume;
//   * lnZ, H and the posterior moments are streamed sums against a running reference exponent R (the largest
//     logw + logl so far): acc = sum exp(term - R) f, rescaled when R grows.
// Everything that decides control flow is workgroup-uniform (counts and flags go through LDS), every sum has a fixed
// order: a star's row depends on its block, the seed and its GLOBAL index only.
// -------------------------------------------------------------------------------------------
namespace iso {
namespace nestk {

using fastk::CoopLds;
using fastk::f_inf;
using fastk::f_nan;

constexpr uint32_t NESTED_TAG = 0x4Eu;        // neither 0x51 (sampler) nor 0x57 (start points)
constexpr int CALLS_PER_CHUNK = 8;            // Philox calls reserved per chunk (5 used at most: 4 pairs of normals + the radius)
constexpr int MAX_D = ISO_NESTED_MAX_D;       // 7: triples
constexpr int NESTED_LDS_LIMIT = 160 * 1024;  // bytes of LDS one workgroup may ask for on gfx950

struct NestedArgs {
    const int64_t* gidx;   // [n_stars] global star index (the random stream's key; the row's position does not enter)
    double* rows;          // [n_stars][2 D + 8]: mean, std per parameter | lnZ lnZ_err H ncall niter prior_fraction status ok
    double* dead;          // [n_stars][max_dead][D + 2]: u, logl, logw + logl - or null
    int32_t* n_dead;       // [n_stars] - or null
    double* trace;         // [n_stars][max_steps][3 + D + D D]: thr[K - 1], first draw, last draw, mean, A (row-major) - or null
    int32_t* n_steps;      // [n_stars] - or null
    int64_t n_stars;
    int nlive, K;
    int max_iter, max_fill_chunks, max_chunks;
    int max_dead, max_steps;
    double ln_tol, enlarge_root;     // ln(evidence_tolerance), enlarge^(1 / D)
    uint64_t seed;
};

// doubles of LDS behind the axes blob and the cooperative-gather slots
__host__ __device__ constexpr int nested_extra_doubles(int nlive, int K, int D)
{
    return BLOCK /* keys */ + 64 /* mean, counters, state */ + 2 * 64 /* L, A */ + BLOCK /* partial sums */ + 3 * K /* csum, term, weight */ +
           K * (D + 1) + 2 * nlive * (D + 1);
}
__host__ __device__ constexpr size_t nested_lds_bytes(int axes_len, int nb, int nlive, int K, int D)
{
    return (size_t)(((axes_len + 1) & ~1) + fastk::coop_lds_doubles(nb) + nested_extra_doubles(nlive, K, D)) * sizeof(double);
}
__host__ __device__ constexpr int nested_K(int nlive, int D)
{
    const int k = nlive / 10, cap = nlive - 2 * (D + 1);
    return k < cap ? (k < 1 ? 1 : k) : cap;
}

__device__ __forceinline__ double block_max(double v, double* buf, int tid)
{
    buf[tid] = v;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) buf[tid] = fmax(buf[tid], buf[tid + s]);
        __syncthreads();
    }
    const double r = buf[0];
    __syncthreads();
    return r;
}

template <int KIND, int NS, int NB>
__global__ __launch_bounds__(BLOCK, 2) void k_catalog_nested(const FastArgs A, const NestedArgs T)
{
    extern __shared__ double lds[];
    constexpr int D = NS + 4, REC = D + 1, NCOV = D * (D + 1) / 2, NACC = 2 * D + 2;
    constexpr int GC = BLOCK / NCOV, GM = BLOCK / D;       // lanes per covariance entry / per mean entry
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < A.axes_len; j += BLOCK) lds[j] = A.axes_blob[j];
    const CoopLds L = fastk::coop_lds<NB>(lds, A.axes_len);
    const int nlive = T.nlive, K = T.K;
    double* keys = lds + ((A.axes_len + 1) & ~1) + fastk::coop_lds_doubles(NB);
    double* st = keys + BLOCK;                 // [0, 8): mean | 8 ..: see below
    double* Lm = st + 64;                      // Cholesky factor of the survivors' covariance, row-major [D][D]
    double* Am = Lm + 64;                      // the ellipsoid's factor: Lm * radius * enlarge^(1 / D)
    double* part = Am + 64;                    // partial sums of the reductions
    double* csum = part + BLOCK;               // csum[j] = sum_{i <= j} 1 / (nlive - i)
    double* term = csum + K;                   // logw + logl of the points being retired
    double* wgt = term + K;                    // exp(term - R)
    double* newbuf = wgt + K;                  // [K][REC] accepted draws of the macro-step, in draw order
    double* live = newbuf + K * REC;           // [2][nlive][REC]: u, logl - sorted ascending in logl
    // st slots: 8 .. 11 wave counts (good), 12 .. 15 wave counts (inside), 16 S0 broadcast, 17 last draw, 18 .. 18 + NACC accumulators
    const int64_t star = blockIdx.x;
    const int64_t gidx = T.gidx[star];
    const DevModel& M = A.m[star];
    const DevModel& MP = A.shared_priors ? A.m[0] : M;
    double lo[D], span[D];
#pragma unroll
    for (int q = 0; q < D; ++q) {
        lo[q] = M.bound_lo[q];
        span[q] = M.bound_hi[q] - lo[q];
    }
    __syncthreads();

    const uint32_t k0 = (uint32_t)T.seed, k1 = (uint32_t)(T.seed >> 32);
    const uint32_t c1 = (uint32_t)gidx, c2 = (uint32_t)tid | ((uint32_t)((uint64_t)gidx >> 32) << 16);
    int chunk = 0, held = 0, cur = 0, it = 0, ndead = 0, nstep = 0, status = 0, fill_chunks = 0;
    bool filling = true;
    double ncall = 0.0, nfinite = 0.0, thr = -f_inf(), logx = 0.0, R = -f_inf(), first_draw = 0.0, frac = 0.0;
    double acc = 0.0;                          // lane q < NACC: its streamed sum (0: 1, 1: logl, 2 ..: theta, 2 + D ..: theta^2)
    double* drow = T.dead ? T.dead + star * (int64_t)T.max_dead * (D + 2) : nullptr;
    double* trow = T.trace ? T.trace + star * (int64_t)T.max_steps * (3 + D + D * D) : nullptr;

    // retire the n points kept[0 .. n) (ascending) with shrinkage 1 / (n_at - j), cs = the running sums of those
    auto retire = [&](const double* kept, int n, const double* cs, double* tm, double* wg, bool last_takes_all) {
        double mx = -f_inf();
        for (int j = tid; j < n; j += BLOCK) {
            const double prev = j == 0 ? logx : logx - cs[j - 1];
            const double lx = (last_takes_all && j == n - 1) ? -f_inf() : logx - cs[j];
            const double t = prev + log1p(-exp(lx - prev)) + kept[j * REC + D];
            tm[j] = t;
            mx = fmax(mx, t);
        }
        const double Rn = fmax(R, block_max(mx, keys, tid));
        for (int j = tid; j < n; j += BLOCK) wg[j] = exp(tm[j] - Rn);
        __syncthreads();
        if (tid < NACC) {
            double a = R > -f_inf() ? acc * exp(R - Rn) : 0.0;
            const int q = tid < 2 + D ? tid - 2 : tid - 2 - D;
            for (int j = 0; j < n; ++j) {
                double f = 1.0;
                if (tid == 1) f = kept[j * REC + D];
                else if (tid >= 2) {
                    double th = 0.0;
#pragma unroll
                    for (int p = 0; p < D; ++p) th = (p == q) ? fma(span[p], kept[j * REC + p], lo[p]) : th;
                    f = tid < 2 + D ? th : th * th;
                }
                a = fma(wg[j], f, a);
            }
            acc = a;
        }
        if (drow) {
            for (int e = tid; e < n * (D + 2); e += BLOCK) {
                const int j = e / (D + 2), q = e - j * (D + 2);
                if (ndead + j < T.max_dead) drow[(int64_t)(ndead + j) * (D + 2) + q] = q <= D ? kept[j * REC + q] : tm[j];
            }
        }
        ndead += n;
        R = Rn;
        __syncthreads();
    };

    for (;;) {
        if (chunk >= (filling ? T.max_fill_chunks : T.max_chunks)) {
            status = filling ? 1 : 2;
            break;
        }
        // ---- one chunk: a draw per lane ----
        double u[D];
        bool inside = true;
        if (filling) {
#pragma unroll
            for (int c = 0; c < (D + 1) / 2; ++c) {
                uint32_t r[4];
                fastk::philox4x32_10((uint32_t)(CALLS_PER_CHUNK * chunk + c), c1, c2, NESTED_TAG, k0, k1, r);
                u[2 * c] = fastk::uniform53(r[0], r[1]);
                if (2 * c + 1 < D) u[2 * c + 1] = fastk::uniform53(r[2], r[3]);
            }
        } else {
            double z[D + 1], n2 = 0.0;
#pragma unroll
            for (int c = 0; c < (D + 1) / 2; ++c) {
                uint32_t r[4];
                fastk::philox4x32_10((uint32_t)(CALLS_PER_CHUNK * chunk + c), c1, c2, NESTED_TAG, k0, k1, r);
                const double rho = sqrt(-2.0 * log(1.0 - fastk::uniform53(r[0], r[1])));
                double sn, cs;
                sincospi(2.0 * fastk::uniform53(r[2], r[3]), &sn, &cs);
                z[2 * c] = rho * cs;
                z[2 * c + 1] = rho * sn;
            }
#pragma unroll
            for (int q = 0; q < D; ++q) n2 = fma(z[q], z[q], n2);
            uint32_t r[4];
            fastk::philox4x32_10((uint32_t)(CALLS_PER_CHUNK * chunk + 4), c1, c2, NESTED_TAG, k0, k1, r);
            const double sc = exp(log(fastk::uniform53(r[0], r[1])) * (1.0 / D)) / sqrt(n2);
#pragma unroll
            for (int q = 0; q < D; ++q) z[q] *= sc;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double x = st[i];
#pragma unroll
                for (int j = 0; j <= i; ++j) x = fma(Am[i * D + j], z[j], x);
                u[i] = x;
                inside = inside && (x >= 0.0) && (x <= 1.0);
            }
        }
        double p[D];
#pragma unroll
        for (int q = 0; q < D; ++q) p[q] = fma(span[q], inside ? u[q] : 0.5, lo[q]);
        double lnp_unused, lnl_unused;
        const double r = fastk::lnpost_wave<KIND, NS, NB, false, true>(A, lds, L, inside, M, MP, p, false, lnp_unused, lnl_unused);
        const bool good = inside && isfinite(r) && (filling || r > thr);
        // ---- taken in draw order: position = held + #{good lanes before this one} ----
        const unsigned long long bg = __ballot(good), bi = __ballot(inside);
        if (lane == 0) {
            st[8 + wave] = (double)__popcll(bg);
            st[12 + wave] = (double)__popcll(bi);
        }
        __syncthreads();
        int before = __popcll(bg & ((1ull << lane) - 1ull)), total = 0, n_in = 0;
        for (int w = 0; w < BLOCK / 64; ++w) {
            const int c = (int)st[8 + w];
            before += w < wave ? c : 0;
            total += c;
            n_in += (int)st[12 + w];
        }
        const int target = filling ? nlive : K;
        const int slot = held + before;
        if (good && slot < target) {
            double* dst = (filling ? live : newbuf) + slot * REC;
#pragma unroll
            for (int q = 0; q < D; ++q) dst[q] = u[q];
            dst[D] = r;
            if (slot == target - 1) st[17] = (double)chunk * BLOCK + tid;
        }
        ncall += filling ? (double)BLOCK : (double)n_in;
        if (filling) nfinite += total;
        held = min(target, held + total);
        ++chunk;
        __syncthreads();
        if (held < target) continue;

        // ---- the list is complete: put it in order ----
        if (filling) {
            fill_chunks = chunk;
            frac = nfinite / ((double)fill_chunks * BLOCK);
            double* dst = live + nlive * REC;
            for (int j = tid; j < nlive; j += BLOCK) {
                const double key = live[j * REC + D];
                int rank = 0;
                for (int i = 0; i < nlive; ++i) {
                    const double v = live[i * REC + D];
                    rank += (int)((v < key) | ((v == key) & (i < j)));
                }
#pragma unroll
                for (int q = 0; q < REC; ++q) dst[rank * REC + q] = live[j * REC + q];
            }
            if (tid == 0) {
                double s = 0.0;
                for (int j = 0; j < K; ++j) {
                    s += 1.0 / (double)(nlive - j);
                    csum[j] = s;
                }
            }
            cur = 1;
            filling = false;
        } else {
            const double* kc = live + cur * nlive * REC + K * REC;      // the survivors
            double* kn = live + (cur ^ 1) * nlive * REC;
            const int ns = nlive - K;
            if (tid == 0 && trow && nstep - 1 < T.max_steps) {
                double* t = trow + (int64_t)(nstep - 1) * (3 + D + D * D);
                t[1] = first_draw;
                t[2] = st[17];
            }
            for (int j = tid; j < K; j += BLOCK) {
                const double key = newbuf[j * REC + D];
                int rank = 0;
                for (int i = 0; i < K; ++i) {
                    const double v = newbuf[i * REC + D];
                    rank += (int)((v < key) | ((v == key) & (i < j)));
                }
                int a = 0, b = ns;                         // first survivor above key (survivors win ties: they are older)
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if (kc[mid * REC + D] <= key) a = mid + 1;
                    else b = mid;
                }
                rank += a;
#pragma unroll
                for (int q = 0; q < REC; ++q) kn[rank * REC + q] = newbuf[j * REC + q];
            }
            for (int i = tid; i < ns; i += BLOCK) {
                const double key = kc[i * REC + D];
                int rank = i;
                for (int j = 0; j < K; ++j) rank += (int)(newbuf[j * REC + D] < key);
#pragma unroll
                for (int q = 0; q < REC; ++q) kn[rank * REC + q] = kc[i * REC + q];
            }
            cur ^= 1;
        }
        __syncthreads();

        // ---- macro-step: retire the K lowest ----
        const double* kc = live + cur * nlive * REC;
        retire(kc, K, csum, term, wgt, false);
        thr = kc[(K - 1) * REC + D];
        logx -= csum[K - 1];
        it += K;
        if (tid == 0) st[16] = acc;
        __syncthreads();
        const double lnz = R + log(st[16]);
        if (kc[(nlive - 1) * REC + D] + logx < lnz + T.ln_tol || it >= T.max_iter) break;

        // ---- bounding ellipsoid of the survivors ----
        const double* sv = kc + K * REC;
        const int ns = nlive - K;
        if (tid < GM * D) {                                 // mean: GM lanes per coordinate, then a sum in lane order
            const int q = tid / GM, g = tid - q * GM;
            double s = 0.0;
            for (int i = g; i < ns; i += GM) s += sv[i * REC + q];
            part[tid] = s;
        }
        __syncthreads();
        if (tid < D) {
            double s = 0.0;
            for (int g = 0; g < GM; ++g) s += part[tid * GM + g];
            st[tid] = s / (double)ns;
        }
        __syncthreads();
        if (tid < GC * NCOV) {                              // covariance (lower triangle): GC lanes per entry
            const int e = tid / GC, g = tid - e * GC;
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= e) ++a;
            const int b = e - a * (a + 1) / 2;
            const double ma = st[a], mb = st[b];
            double s = 0.0;
            for (int i = g; i < ns; i += GC) s = fma(sv[i * REC + a] - ma, sv[i * REC + b] - mb, s);
            part[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double* C = Am;                                  // (the factor's storage until the factor is known)
            for (int a = 0; a < D; ++a)
                for (int b = 0; b < D; ++b) {
                    const int e = a * (a + 1) / 2 + b;
                    double s = 0.0;
                    if (b <= a)
                        for (int g = 0; g < GC; ++g) s += part[e * GC + g];
                    C[a * D + b] = b <= a ? s / (double)(ns - 1) + (a == b ? 1e-14 : 0.0) : 0.0;
                    Lm[a * D + b] = 0.0;
                }
            bool ok = true;
            for (int a = 0; a < D && ok; ++a)
                for (int b = 0; b <= a; ++b) {
                    double s = C[a * D + b];
                    for (int k = 0; k < b; ++k) s -= Lm[a * D + k] * Lm[b * D + k];
                    if (a == b) {
                        ok = s > 0.0;
                        Lm[a * D + a] = sqrt(s);
                    } else Lm[a * D + b] = s / Lm[b * D + b];
                }
            if (!ok)                                         // not positive definite: the diagonal, as _bounding_ellipsoid does
                for (int a = 0; a < D; ++a)
                    for (int b = 0; b < D; ++b) Lm[a * D + b] = a == b ? sqrt(C[a * D + a]) : 0.0;
        }
        __syncthreads();
        double r2 = 0.0;
        for (int i = tid; i < ns; i += BLOCK) {              // largest Mahalanobis distance: forward substitution per point
            double y[D], s2 = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                double s = sv[i * REC + a] - st[a];
#pragma unroll
                for (int b = 0; b < a; ++b) s -= Lm[a * D + b] * y[b];
                y[a] = s / Lm[a * D + a];
                s2 = fma(y[a], y[a], s2);
            }
            r2 = fmax(r2, s2);
        }
        r2 = block_max(r2, keys, tid);
        const double f = sqrt(r2) * T.enlarge_root;
        if (tid < D * D) Am[tid] = Lm[tid] * f;
        first_draw = (double)chunk * BLOCK;
        __syncthreads();
        if (trow && nstep < T.max_steps) {
            double* t = trow + (int64_t)nstep * (3 + D + D * D);
            if (tid == 0) t[0] = thr;
            if (tid < D) t[3 + tid] = st[tid];
            if (tid < D * D) t[3 + D + tid] = Am[tid];
        }
        ++nstep;
        held = 0;
    }

    // ---- finish ----
    if (status == 0) {
        const int n_left = nlive - K;
        const double* sv = live + cur * nlive * REC + K * REC;
        double* other = live + (cur ^ 1) * nlive * REC;      // free now: running sums, terms and weights of the last sweep
        if (tid == 0) {
            double s = 0.0;
            for (int j = 0; j < n_left; ++j) {
                s += 1.0 / (double)(n_left - j);
                other[j] = s;
            }
        }
        __syncthreads();
        retire(sv, n_left, other, other + n_left, other + 2 * n_left, true);
    }
    if (tid < NACC) st[18 + tid] = acc;
    __syncthreads();
    double* row = T.rows + star * (int64_t)(2 * D + 8);
    const bool ok = status == 0;
    if (tid < D) {
        const double s0 = st[18], m = st[20 + tid] / s0, v = st[20 + D + tid] / s0 - m * m;
        row[2 * tid] = ok ? m : f_nan();
        row[2 * tid + 1] = ok ? sqrt(fmax(v, 0.0)) : f_nan();
    }
    if (tid == 0) {
        const double s0 = st[18], lnz0 = R + log(s0), H = fmax(st[19] / s0 - lnz0, 0.0);
        double* o = row + 2 * D;
        o[0] = ok ? lnz0 + log(frac) : f_nan();
        o[1] = ok ? sqrt(H / (double)nlive) : f_nan();
        o[2] = ok ? H : f_nan();
        o[3] = ncall;
        o[4] = (double)it;
        o[5] = ok ? frac : (fill_chunks ? frac : nfinite / fmax((double)chunk * BLOCK, 1.0));
        o[6] = (double)status;
        o[7] = ok ? 1.0 : 0.0;
        if (T.n_dead) T.n_dead[star] = ok ? min(ndead, T.max_dead) : 0;
        if (T.n_steps) T.n_steps[star] = min(nstep, T.max_steps);
    }
}

}  // namespace nestk
}  // namespace iso
