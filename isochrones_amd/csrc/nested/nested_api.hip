// C ABI of libiso_nested.so (include/isochrones_amd_nested.h): argument checks and the dispatch to the launchers
#include <cstdio>

#include "nested_launch.h"

namespace {
thread_local std::string g_error;
thread_local std::string g_kernel;

int nfail(int code, const std::string& msg)
{
    g_error = msg;
    return code;
}
}  // namespace

namespace iso {
namespace nestk {
void note_nested_kernel(int kind, int ns, int nb)
{
    char buf[96];
    std::snprintf(buf, sizeof buf, "k_catalog_nested<%d, %d, %d>", kind, ns, nb);
    g_kernel = buf;
}
}  // namespace nestk
}  // namespace iso

using namespace iso;
using namespace iso::nestk;

extern "C" {

const char* iso_nested_version(void) { return "isochrones_amd nested 1 (gfx950)"; }
const char* iso_nested_last_error(void) { return g_error.c_str(); }
const char* iso_nested_last_kernel(void) { return g_kernel.c_str(); }
size_t iso_nested_fast_args_size(void) { return sizeof(FastArgs); }

int iso_nested_remove(int n_live, int n_stars_per_system)
{
    if (n_stars_per_system < 1 || n_stars_per_system > 3 || n_live < 1) return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_remove: bad argument");
    return nested_K(n_live, n_stars_per_system + 4);
}

int iso_nested_max_live(int n_stars_per_system, int n_bands, int axes_len)
{
    if (n_stars_per_system < 1 || n_stars_per_system > 3 || n_bands < 1 || n_bands > ISO_NESTED_MAX_BANDS || axes_len < 0)
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_max_live: 1-3 stars, 1-12 bands");
    const int D = n_stars_per_system + 4;
    int lo = 0, hi = 1 << 16;                        // nested_lds_bytes grows with n_live: the largest that fits, by bisection
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (nested_lds_bytes(axes_len, n_bands, mid, nested_K(mid, D), D) <= (size_t)NESTED_LDS_LIMIT) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

int iso_nested_max_live_catalog(const void* fast_args, size_t fast_args_size, int n_stars_per_system, int n_bands)
{
    if (!fast_args || fast_args_size != sizeof(FastArgs))
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_max_live_catalog: not this library's kernel-argument block");
    FastArgs A;
    std::memcpy(&A, fast_args, sizeof A);
    return iso_nested_max_live(n_stars_per_system, n_bands, A.axes_len);
}

int iso_nested_fit(const void* fast_args, size_t fast_args_size, int kind, int n_stars_per_system, int n_bands,
                   int64_t n_models, const int64_t* global_index, int n_live, double evidence_tolerance, double enlarge,
                   uint64_t seed, int max_iter, int max_fill_chunks, int max_chunks, double* rows, double* dead,
                   int32_t* n_dead, int max_dead, double* trace, int32_t* n_steps, int max_steps, void* stream)
{
    if (!fast_args || !global_index || !rows) return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: NULL argument");
    if (fast_args_size != sizeof(FastArgs))
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: the kernel-argument block has another size than this library's (stale build?)");
    if (kind != ISO_KIND_TRACK && kind != ISO_KIND_ISO) return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: unknown parametrisation");
    if (n_stars_per_system < 1 || n_stars_per_system > 3 || (kind == ISO_KIND_TRACK && n_stars_per_system != 1) || n_bands < 1 ||
        n_bands > ISO_NESTED_MAX_BANDS)
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: no kernel for this shape (1-3 stars on the isochrone grid, 1 on the track grid, 1-12 bands)");
    if (n_models < 1 || n_models > 0x7fffffff) return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: n_models out of range");
    const int D = n_stars_per_system + 4;
    if (n_live < (20 > 4 * (D + 1) ? 20 : 4 * (D + 1))) return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: n_live below max(20, 4 (D + 1))");
    if (!(evidence_tolerance > 0.0) || !(enlarge >= 1.0)) return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: evidence_tolerance must be positive, enlarge at least 1");
    if (max_iter < 1 || max_fill_chunks < 1 || max_chunks < 1 || max_chunks > (1 << 28))
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: max_iter, max_fill_chunks and max_chunks must be positive (max_chunks at most 2^28)");
    if ((dead != nullptr) != (n_dead != nullptr) || (dead && max_dead < 1) || (trace != nullptr) != (n_steps != nullptr) || (trace && max_steps < 1))
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: dead / n_dead and trace / n_steps come in pairs, with positive capacities");
    FastArgs A;
    std::memcpy(&A, fast_args, sizeof A);
    if (!A.hotq || !A.bcq || !A.m || !A.axes_blob || A.axes_len < 1 || A.axes_len > MAX_LDS_AXIS_DOUBLES)
        return nfail(ISO_NESTED_ERR_INVALID, "iso_nested_fit: the block is not a corner-packed catalog's");
    const int cap = iso_nested_max_live(n_stars_per_system, n_bands, A.axes_len);
    if (n_live > cap) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "iso_nested_fit: n_live %d above the %d that fit a workgroup's LDS for this shape", n_live, cap);
        return nfail(ISO_NESTED_ERR_INVALID, buf);
    }
    NestedArgs T;
    T.gidx = global_index;
    T.rows = rows;
    T.dead = dead;
    T.n_dead = n_dead;
    T.trace = trace;
    T.n_steps = n_steps;
    T.n_stars = n_models;
    T.nlive = n_live;
    T.K = nested_K(n_live, D);
    T.max_iter = max_iter;
    T.max_fill_chunks = max_fill_chunks < max_chunks ? max_fill_chunks : max_chunks;
    T.max_chunks = max_chunks;
    T.max_dead = max_dead;
    T.max_steps = max_steps;
    T.ln_tol = std::log(evidence_tolerance);
    T.enlarge_root = std::pow(enlarge, 1.0 / D);
    T.seed = seed;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool hi = n_bands > 6;
    int rc;
    if (kind == ISO_KIND_TRACK) rc = hi ? launch_nested_track1_hi(n_bands, A, T, s) : launch_nested_track1_lo(n_bands, A, T, s);
    else if (n_stars_per_system == 1) rc = hi ? launch_nested_iso1_hi(n_bands, A, T, s) : launch_nested_iso1_lo(n_bands, A, T, s);
    else if (n_stars_per_system == 2) rc = hi ? launch_nested_iso2_hi(n_bands, A, T, s) : launch_nested_iso2_lo(n_bands, A, T, s);
    else rc = hi ? launch_nested_iso3_hi(n_bands, A, T, s) : launch_nested_iso3_lo(n_bands, A, T, s);
    if (rc != 0) return nfail(rc, rc == ISO_NESTED_ERR_HIP ? "iso_nested_fit: the launch failed" : "iso_nested_fit: no kernel for this shape");
    return 0;
}

}  // extern "C"
