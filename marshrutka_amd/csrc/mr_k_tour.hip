// mr_k_tour.hip — tour plans' reduction kernel (tour_kernel)
// (host-side launch helpers called from mr_host.cpp; device code in mr_tour.hpp)
#include "mr_tour.hpp"

namespace mr {

template <bool WAVE>
static const void *tour_fn(const uint32_t perm[3]) {
    switch (perm[0] * 9 + perm[1] * 3 + perm[2]) {
        case 5: return (const void *)&tour_kernel<5, WAVE>;
        case 7: return (const void *)&tour_kernel<7, WAVE>;
        case 11: return (const void *)&tour_kernel<11, WAVE>;
        case 15: return (const void *)&tour_kernel<15, WAVE>;
        case 19: return (const void *)&tour_kernel<19, WAVE>;
        case 21: return (const void *)&tour_kernel<21, WAVE>;
        default: return nullptr;
    }
}

// LDS of a workgroup for tours of at most nmax stops: a slot a wave, or one
uint32_t tour_lds_bytes(uint32_t nmax, bool wave) { return 4u * tour_slot_words(nmax) * (wave ? kBS / 64 : 1); }

// more than 64 KB of dynamic LDS needs the function's attribute raised first
static hipError_t tour_lds_attr(const void *fn, uint32_t bytes) {
    if (bytes <= 64u * 1024u) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
}

// wave: a wave a tour (four a workgroup), else a workgroup a tour
hipError_t launch_tour(const TourArgs &ta, const uint32_t perm[3], bool wave, uint32_t gx, hipStream_t stream) {
    const void *fn = wave ? tour_fn<true>(perm) : tour_fn<false>(perm);
    if (!fn) return hipErrorInvalidValue;
    const uint32_t bytes = tour_lds_bytes(ta.nmax, wave);
    if (const hipError_t e = tour_lds_attr(fn, bytes)) return e;
    TourArgs copy = ta;
    void *args[] = {&copy};
    return hipLaunchKernel(fn, dim3(gx), dim3(kBS), args, bytes, stream);
}

// resident tour workgroups per CU at that LDS: the grid is at most one round of them
int tour_blocks_per_cu(const uint32_t perm[3], bool wave, uint32_t nmax) {
    const void *fn = wave ? tour_fn<true>(perm) : tour_fn<false>(perm);
    int n = 0;
    const uint32_t bytes = tour_lds_bytes(nmax, wave);
    if (fn && tour_lds_attr(fn, bytes) == hipSuccess) n = occupancy_cached(fn, kBS, bytes);
    return n;
}

}  // namespace mr
