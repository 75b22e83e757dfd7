// mr_k_nearest_src.hip — nearest-source plans' reduction kernels (nearest_src_kernel,
// nearest_src_merge_kernel)
// (host-side launch helpers called from mr_host.cpp; device code in mr_nearest_src.hpp)
#include "mr_nearest_src.hpp"

namespace mr {

template <bool WORST, bool MERGE>
static const void *nearest_src_fn(const uint32_t perm[3]) {
#define MR_NSRC_CASE(P) \
    case P: return MERGE ? (const void *)&nearest_src_merge_kernel<P, WORST> : (const void *)&nearest_src_kernel<P, WORST>;
    switch (perm[0] * 9 + perm[1] * 3 + perm[2]) {
        MR_NSRC_CASE(5)
        MR_NSRC_CASE(7)
        MR_NSRC_CASE(11)
        MR_NSRC_CASE(15)
        MR_NSRC_CASE(19)
        MR_NSRC_CASE(21)
        default: return nullptr;
    }
#undef MR_NSRC_CASE
}

static const void *nearest_src_pick(const uint32_t perm[3], bool worst, bool merge) {
    if (merge) return worst ? nearest_src_fn<true, true>(perm) : nearest_src_fn<false, true>(perm);
    return worst ? nearest_src_fn<true, false>(perm) : nearest_src_fn<false, false>(perm);
}

// the reduction over gx workgroups, a wave an item
hipError_t launch_nearest_src(const NearestSrcArgs &na, const uint32_t perm[3], bool worst, uint32_t gx, hipStream_t stream) {
    const void *fn = nearest_src_pick(perm, worst, false);
    if (!fn) return hipErrorInvalidValue;
    NearestSrcArgs copy = na;
    void *args[] = {&copy};
    return hipLaunchKernel(fn, dim3(gx), dim3(kBS), args, 0, stream);
}

// the merge of the split groups' slabs, a lane a (destination, split group)
hipError_t launch_nearest_src_merge(const NearestSrcArgs &na, const uint32_t perm[3], bool worst, hipStream_t stream) {
    const void *fn = nearest_src_pick(perm, worst, true);
    if (!fn) return hipErrorInvalidValue;
    const unsigned long long lanes = (unsigned long long)na.n_split * na.pitch;
    NearestSrcArgs copy = na;
    void *args[] = {&copy};
    return hipLaunchKernel(fn, dim3(uint32_t((lanes + kBS - 1) / kBS)), dim3(kBS), args, 0, stream);
}

// an item a wave: the waves of a workgroup
uint32_t nearest_src_waves_per_block() { return kBS / 64; }

int nearest_src_blocks_per_cu(const uint32_t perm[3], bool worst) {
    const void *fn = nearest_src_pick(perm, worst, false);
    int n = 0;
    if (fn) n = occupancy_cached(fn, kBS, 0);
    return n;
}

}  // namespace mr
