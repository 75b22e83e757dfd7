// mr_k_matrix.hip — matrix plans' read-off kernel (matrix_kernel)
// (host-side launch helpers called from mr_host.cpp; device code in mr_matrix.hpp)
#include "mr_matrix.hpp"

namespace mr {

static const void *matrix_fn(const uint32_t perm[3]) {
    switch (perm[0] * 9 + perm[1] * 3 + perm[2]) {
        case 5: return (const void *)&matrix_kernel<5>;
        case 7: return (const void *)&matrix_kernel<7>;
        case 11: return (const void *)&matrix_kernel<11>;
        case 15: return (const void *)&matrix_kernel<15>;
        case 19: return (const void *)&matrix_kernel<19>;
        case 21: return (const void *)&matrix_kernel<21>;
        default: return nullptr;
    }
}

hipError_t launch_matrix(const KArgs *d_args, const uint32_t perm[3], uint32_t gx, hipStream_t stream) {
    const void *fn = matrix_fn(perm);
    if (!fn) return hipErrorInvalidValue;
    void *args[] = {const_cast<KArgs **>(&d_args)};
    return hipLaunchKernel(fn, dim3(gx), dim3(kBS), args, 0, stream);
}

// resident matrix workgroups per CU: the grid is at most one round of them
int matrix_blocks_per_cu(const uint32_t perm[3]) {
    const void *fn = matrix_fn(perm);
    int n = 0;
    if (fn) n = occupancy_cached(fn, kBS, 0);
    return n;
}

}  // namespace mr
