// launchers of k_catalog_nested: one translation unit per (parametrisation, stars, half of the band range)
#pragma once
#include "nested_kernel.h"

namespace iso {
namespace nestk {

// the name of the instantiation a launcher chose (iso_nested_last_kernel)
void note_nested_kernel(int kind, int ns, int nb);

template <int KIND, int NS, int NB>
inline int launch_nested_one(const FastArgs& A, const NestedArgs& T, hipStream_t s)
{
    const size_t sh = nested_lds_bytes(A.axes_len, NB, T.nlive, T.K, NS + 4);
    if (sh > (size_t)NESTED_LDS_LIMIT) return ISO_NESTED_ERR_INVALID;
    if (sh > 64 * 1024 &&                            // beyond what a launch gets without asking
        hipFuncSetAttribute((const void*)k_catalog_nested<KIND, NS, NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh) != hipSuccess)
        return ISO_NESTED_ERR_HIP;
    hipLaunchKernelGGL((k_catalog_nested<KIND, NS, NB>), dim3((unsigned)T.n_stars), dim3(BLOCK), sh, s, A, T);
    if (hipGetLastError() != hipSuccess) return ISO_NESTED_ERR_HIP;
    note_nested_kernel(KIND, NS, NB);
    return 0;
}

template <int KIND, int NS, int NB0>
inline int launch_nested_six(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s)
{
    switch (nb - NB0) {
    case 0: return launch_nested_one<KIND, NS, NB0>(A, T, s);
    case 1: return launch_nested_one<KIND, NS, NB0 + 1>(A, T, s);
    case 2: return launch_nested_one<KIND, NS, NB0 + 2>(A, T, s);
    case 3: return launch_nested_one<KIND, NS, NB0 + 3>(A, T, s);
    case 4: return launch_nested_one<KIND, NS, NB0 + 4>(A, T, s);
    case 5: return launch_nested_one<KIND, NS, NB0 + 5>(A, T, s);
    }
    return ISO_NESTED_ERR_INVALID;
}

#define ISO_DEFINE_NESTED_LAUNCHER(NAME, KIND, NS, NB0)                                       \
    int NAME(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s)                   \
    {                                                                                         \
        return launch_nested_six<KIND, NS, NB0>(nb, A, T, s);                                 \
    }

int launch_nested_track1_lo(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_track1_hi(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_iso1_lo(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_iso1_hi(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_iso2_lo(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_iso2_hi(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_iso3_lo(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);
int launch_nested_iso3_hi(int nb, const FastArgs& A, const NestedArgs& T, hipStream_t s);

}  // namespace nestk
}  // namespace iso
