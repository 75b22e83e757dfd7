// mr_nearest_src.hpp — nearest-source plans: per destination and group of sources the best (or the
// worst) listed source, reduced on the device from the plan's own matrix rows (DESIGN.md section
// 3b''''').
//
// The matrix pass before these launches on the stream has written a 16 B record per (plan source,
// destination), destinations in the caller's order.  The sources are stable-sorted by group; the
// host cuts each group into segments of consecutive sorted sources (one segment unless the
// destination chunks x groups leave wave slots empty).
//
//   nearest_src_kernel        a wave an item = (segment, 64-destination chunk).  Lane l owns
//                             destination 64 c + l and walks the segment's sources in sorted
//                             order: the row index is wave-uniform, a source costs one 16 B load a
//                             lane (1 KB contiguous a wave), kNsrcUnroll sources' loads are issued
//                             before the first compare.  The running best (three key words, via,
//                             the sorted index) stays in registers and is replaced on a strict
//                             compare only, so the earliest of equals stays.  No cross-lane
//                             exchange, no LDS, no atomic.  A segment that is its whole group
//                             stores the final 32 B record, any other the same 32 B into its slab
//                             of the partials.
//   nearest_src_merge_kernel  a lane a (destination, split group): folds the group's slabs in
//                             segment order, strict again, and stores the final record.
#pragma once
#include "mr_device.hpp"

namespace mr {

constexpr uint32_t kNsrcUnroll = 8u;

template <bool WORST>
__device__ __forceinline__ bool nsrc_better(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2) {
    return WORST ? (a0 > b0 || (a0 == b0 && (a1 > b1 || (a1 == b1 && a2 > b2))))
                 : (a0 < b0 || (a0 == b0 && (a1 < b1 || (a1 == b1 && a2 < b2))));
}

// metric q of a record's words
template <uint32_t Q>
__device__ __forceinline__ uint32_t nsrc_word(const uint4 &r) {
    return Q == 0 ? r.x : (Q == 1 ? r.y : r.z);
}

template <uint32_t PERM, bool WORST>
__global__ __launch_bounds__(kBS) void nearest_src_kernel(const NearestSrcArgs a) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * (kBS / 64), gw = blockIdx.x * (kBS / 64) + wv;
    const uint32_t items = a.n_seg * a.n_chunk;
    for (uint32_t it = gw; it < items; it += nwaves) {
        const uint32_t s = it / a.n_chunk, c = it - s * a.n_chunk;
        const uint4 sg = a.segs[s];  // {first sorted source, sources, group, slab or kNone32}: uniform
        const uint32_t first = uint32_t(__builtin_amdgcn_readfirstlane(int(sg.x)));
        const uint32_t count = uint32_t(__builtin_amdgcn_readfirstlane(int(sg.y)));
        const uint32_t group = uint32_t(__builtin_amdgcn_readfirstlane(int(sg.z)));
        const uint32_t slab = uint32_t(__builtin_amdgcn_readfirstlane(int(sg.w)));
        const uint32_t j = 64u * c + lane;
        // a lane past the last destination reads the last one's records and stores nothing
        const uint4 *const col = a.rows + min(j, a.n_dst - 1u);
        const uint32_t *const row_of = a.row_of + first;
        uint4 best = make_uint4(0u, 0u, 0u, 0u);
        uint32_t bk = 0xFFFFFFFFu;  // the winner's sorted index; none yet
        const auto take = [&](const uint4 &r, uint32_t k) {
            const bool t = bk == 0xFFFFFFFFu || nsrc_better<WORST>(nsrc_word<q0>(r), nsrc_word<q1>(r), nsrc_word<q2>(r),
                                                                   nsrc_word<q0>(best), nsrc_word<q1>(best), nsrc_word<q2>(best));
            best.x = t ? r.x : best.x;
            best.y = t ? r.y : best.y;
            best.z = t ? r.z : best.z;
            best.w = t ? r.w : best.w;
            bk = t ? k : bk;
        };
        // The next round's row indices are loaded behind this round's records, so a round waits
        // for one memory latency, not two; row_of ends in 2 * kNsrcUnroll spare entries, so the
        // reads past the segment stay inside the table.  The last round's spare slots load the
        // round's first record again and are not compared.
        uint32_t nxt[kNsrcUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kNsrcUnroll; ++u) nxt[u] = row_of[u];
        for (uint32_t k = 0u; k < count; k += kNsrcUnroll) {
            uint32_t row[kNsrcUnroll];
            uint4 r[kNsrcUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kNsrcUnroll; ++u) row[u] = uint32_t(__builtin_amdgcn_readfirstlane(int(nxt[u])));
#pragma unroll
            for (uint32_t u = 0; u < kNsrcUnroll; ++u) r[u] = col[(unsigned long long)(k + u < count ? row[u] : row[0]) * a.mx_pitch];
#pragma unroll
            for (uint32_t u = 0; u < kNsrcUnroll; ++u) nxt[u] = row_of[k + kNsrcUnroll + u];
#pragma unroll
            for (uint32_t u = 0; u < kNsrcUnroll; ++u)
                if (k + u < count) take(r[u], first + k + u);
        }
        if (j < a.n_dst) {
            const uint32_t pos = bk == 0xFFFFFFFFu ? 0xFFFFFFFFu : a.pos_of[bk];
            uint4 *const out = slab == 0xFFFFFFFFu ? a.records + 2ull * ((unsigned long long)group * a.pitch + j)
                                                   : a.partials + 2ull * ((unsigned long long)slab * a.pitch + j);
            out[0] = best;
            out[1] = make_uint4(pos, 0u, 0u, 0u);
        }
    }
}

template <uint32_t PERM, bool WORST>
__global__ __launch_bounds__(kBS) void nearest_src_merge_kernel(const NearestSrcArgs a) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    const unsigned long long t = (unsigned long long)blockIdx.x * kBS + threadIdx.x;
    const uint32_t m = uint32_t(t / a.pitch), j = uint32_t(t - (unsigned long long)m * a.pitch);
    if (m >= a.n_split || j >= a.n_dst) return;
    const uint4 sp = a.splits[m];  // {group, first slab, slabs, 0}
    const uint4 *p = a.partials + 2ull * ((unsigned long long)sp.y * a.pitch + j);
    uint4 best = make_uint4(0u, 0u, 0u, 0u);
    uint32_t bpos = 0xFFFFFFFFu;
    // kNsrcUnroll slabs' records are loaded before the first compare (a slab costs 32 B a lane)
    const unsigned long long step = 2ull * a.pitch;
    for (uint32_t z = 0; z < sp.z; z += kNsrcUnroll) {
        uint4 r[kNsrcUnroll];
        uint32_t pos[kNsrcUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kNsrcUnroll; ++u) {
            const uint4 *const q = p + step * min(z + u, sp.z - 1u);
            r[u] = q[0];
            pos[u] = q[1].x;
        }
#pragma unroll
        for (uint32_t u = 0; u < kNsrcUnroll; ++u) {
            const bool t2 = z + u < sp.z && pos[u] != 0xFFFFFFFFu &&
                            (bpos == 0xFFFFFFFFu ||
                             nsrc_better<WORST>(nsrc_word<q0>(r[u]), nsrc_word<q1>(r[u]), nsrc_word<q2>(r[u]), nsrc_word<q0>(best),
                                                nsrc_word<q1>(best), nsrc_word<q2>(best)));
            best.x = t2 ? r[u].x : best.x;
            best.y = t2 ? r[u].y : best.y;
            best.z = t2 ? r[u].z : best.z;
            best.w = t2 ? r[u].w : best.w;
            bpos = t2 ? pos[u] : bpos;
        }
    }
    uint4 *const out = a.records + 2ull * ((unsigned long long)sp.x * a.pitch + j);
    out[0] = best;
    out[1] = make_uint4(bpos, 0u, 0u, 0u);
}

}  // namespace mr
