// mr_k_knearest.hip — k-nearest plans' read-off kernel (knearest_kernel)
// (host-side launch helpers called from mr_host.cpp; device code in mr_knearest.hpp)
#include "mr_knearest.hpp"

namespace mr {

static const void *knearest_fn(const uint32_t perm[3]) {
    switch (perm[0] * 9 + perm[1] * 3 + perm[2]) {
        case 5: return (const void *)&knearest_kernel<5>;
        case 7: return (const void *)&knearest_kernel<7>;
        case 11: return (const void *)&knearest_kernel<11>;
        case 15: return (const void *)&knearest_kernel<15>;
        case 19: return (const void *)&knearest_kernel<19>;
        case 21: return (const void *)&knearest_kernel<21>;
        default: return nullptr;
    }
}

hipError_t launch_knearest(const KArgs *d_args, const uint32_t perm[3], uint32_t gx, hipStream_t stream) {
    const void *fn = knearest_fn(perm);
    if (!fn) return hipErrorInvalidValue;
    void *args[] = {const_cast<KArgs **>(&d_args)};
    return hipLaunchKernel(fn, dim3(gx), dim3(kBS), args, 0, stream);
}

// resident k-nearest workgroups per CU: the grid is at most one round of them
int knearest_blocks_per_cu(const uint32_t perm[3]) {
    const void *fn = knearest_fn(perm);
    int n = 0;
    if (fn) n = occupancy_cached(fn, kBS, 0);
    return n;
}

}  // namespace mr
