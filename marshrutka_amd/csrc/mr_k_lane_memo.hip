// mr_k_lane_memo.hip — the lane memo (DESIGN.md section 3a'''): under a comparator order
// that leads with Legs, with caravans and Scrolls of Escape on, the labels of the specials
// depend on a non-special source only through its SoE region.  hub_lane_build_kernel
// solves them once per region and once per special cell (LaneHub<.., kLaneBuild>, one
// wave); hub_lane_memo_kernel is hub_lane_kernel without the own edges and the Dijkstra:
// each lane takes its source's row and reads its destinations off it.  The host decides
// per (grid, params) whether the rows stand for every source (lane_memo_rows, mr_host.cpp).
// hub_lane_win_kernel then finds, once per (region row, cell), the boundary whose walk is
// the best into the cell, and the read-off takes it from that table (lane_win_table).
#include "mr_hub_lane.hpp"

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

namespace mr {

// one wave: lane l solves source l of a->src_v (the first a->nreg of them region
// representatives, then the specials' cells) into row l of a->lane_memo
template <uint32_t PERM, uint32_t TM>
__global__ __launch_bounds__(kBS, lane_waves(TM)) void hub_lane_build_kernel(const KArgs *__restrict__ a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LaneHub<PERM, TM, false, kLaneBuild> H;
    lane_setup<TM>(a, smem, H);
    H.MC = reinterpret_cast<uint32_t *>(smem + lane_lds_total(a->p.NS, a->nreg, TM)) + (threadIdx.x >> 6) * (TM * 64u);
    const uint32_t s_idx = threadIdx.x, n = a->n_lane;
    const bool have = s_idx < n;
    // (whole waves: the Dijkstra's wave-wide tests want every lane in)
    if (__any(have)) H.build_row(have, have ? s_idx : (n ? n - 1 : 0), s_idx < a->nreg);
}

// the memo kernels' LDS: the lane kernels' block without its pair table, then the rows;
// kLaneStage: then a stage per wave
__host__ __device__ inline uint32_t lane_memo_lds_bytes(uint32_t NS, uint32_t nreg, uint32_t TM) {
    return lane_memo_off_rows(NS, nreg, TM) + (nreg + NS) * lane_memo_row_words(TM) * 4u;
}
__host__ __device__ inline uint32_t lane_stage_lds_bytes(uint32_t NS, uint32_t nreg, uint32_t TM) {
    return lane_memo_lds_bytes(NS, nreg, TM) + (kBS / 64) * kLaneStageWave;
}

// The winner table of a gated (grid, params): a thread per cell.  Under the gate the best
// boundary walk into a plain cell depends on the source only through its region row, so it
// is found here once per (row, cell), by the read-off's own candidate and tie loops
// (LaneHub::best_walk) from the row's representative source, a->src_v[r], without that
// source's walk; hub_lane_memo_kernel then compares one boundary's walk with the source's
// own.  a->lane_win: a word per cell; a->lane_reg0: the region row each cell lies in.
template <uint32_t PERM, uint32_t TM>
__global__ __launch_bounds__(kBS, 4) void hub_lane_win_kernel(const KArgs *__restrict__ a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LaneHub<PERM, TM, false, kLaneMemo> H;
    const uint32_t NS = a->p.NS, nreg = a->nreg, V = a->p.S * a->p.S;
    uint4 *rows = reinterpret_cast<uint4 *>(smem + lane_memo_off_rows(NS, nreg, TM));
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(a->lane_memo);
        const uint32_t n16 = (nreg + NS) * (lane_memo_row_words(TM) / 4u);
        for (uint32_t i = threadIdx.x; i < n16; i += kBS) rows[i] = g[i];
    }
    lane_setup<TM, decltype(H), false>(a, smem, H);
    const uint32_t w = blockIdx.x * kBS + threadIdx.x;
    if (w >= V) return;
    {  // the lowest region at distance 0, as memo_solve picks it from the cell's region row
        const uint2 *row = reinterpret_cast<const uint2 *>(a->near) + (unsigned long long)w * nreg;
        uint32_t reg = kLaneRegNone;
        for (uint32_t r = min(nreg, kLaneRegs); r-- > 0;) reg = row[r].x == 0u ? r : reg;
        a->lane_reg0[w] = uint8_t(reg);
    }
    a->lane_win[w] = H.win_word(w, rows);
}

// hub_lane_kernel's launch geometry, source order and end-of-pass bookkeeping.  Four
// waves per SIMD: a lane holds no table, only the destination it is reading off.  MODE
// kLaneMemo: every destination runs the candidates.  MODE kLaneWin: plain sources read
// their destinations' best boundary off the winner table; the candidates stay for the
// special sources, behind a wave-uniform branch, and keep the registers at four waves
// (more waves per SIMD measured slower, DESIGN.md section 3a''').
// MODE kLaneStage: kLaneWin with whole command rows (read_off_staged); three waves per SIMD,
// since at four the stage's few more registers would go to scratch memory.
#ifndef MR_LANE_STAGE_WAVES
#define MR_LANE_STAGE_WAVES 3
#endif
// kLaneQuery: the chunks a wave's source cells and destinations are loaded ahead of the chunk
// it reads off (2; 1: in the iteration that issues the gathers they address, for the A/B of
// DESIGN.md section 3a''')
#ifndef MR_LANE_QUERY_DEPTH
#define MR_LANE_QUERY_DEPTH 2
#endif
template <uint32_t PERM, uint32_t TM, uint32_t MODE>
__global__ __launch_bounds__(kBS, MODE == kLaneStage ? MR_LANE_STAGE_WAVES : 4) void hub_lane_memo_kernel(const KArgs *__restrict__ a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LaneHub<PERM, TM, false, MODE> H;
#ifdef MR_STAMPS
    H.lst_last = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t NS = a->p.NS, nreg = a->nreg;
    uint4 *rows = reinterpret_cast<uint4 *>(smem + lane_memo_off_rows(NS, nreg, TM));
    {  // (before lane_setup's barrier; L2-resident after the first workgroups)
        const uint4 *g = reinterpret_cast<const uint4 *>(a->lane_memo);
        const uint32_t n16 = (nreg + NS) * (lane_memo_row_words(TM) / 4u);
        for (uint32_t i = threadIdx.x; i < n16; i += kBS) rows[i] = g[i];
    }
    lane_setup<TM, decltype(H), false>(a, smem, H);
#ifdef MR_STAMPS
    {
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();
        H.lst[0] += now_ - H.lst_last;  // (0: the table copy)
        H.lst_last = now_;
    }
#endif
    const uint32_t s_idx = (blockIdx.x * (kBS / 64) + (threadIdx.x >> 6)) * 64u + lane_id();
    uint32_t written = 0;
    if constexpr (MODE == kLaneQuery) {
        // A record per lane, persistent waves: the launch's waves walk the chunks of 64
        // records at a grid-wide stride, so the chunks in flight are neighbours in the
        // output.  A chunk's source cells and destinations (coalesced) and then its two
        // gathers (the source's region byte, the destination's winner word) are issued
        // one chunk ahead of the chunk whose destinations are read off and stored, and the
        // source cells and destinations that address them two chunks ahead: a chunk's
        // iteration issues the indices of the chunk after next, then the next chunk's
        // gathers from the indices the iteration before loaded, so no load is waited for
        // in the iteration that issued it.  Every load is issued by every lane, a lane
        // without a record (the plan's last chunk, a look-ahead past the wave's last
        // chunk) taking the plan's last record: with the loads behind no branch and the
        // stores one block per chunk (LaneHub::emit_q), the waits are counted ones and
        // leave the chunk's stores in flight.
        const uint32_t nq = a->nq_lane, chunks = (nq + 63u) / 64u, nw = gridDim.x * (kBS / 64);
        const uint32_t *qsv = a->q_srcv, *qd = a->q_dst, *win = a->lane_win;
        const uint8_t *reg0 = a->lane_reg0;
        uint32_t c = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBS / 64) + (threadIdx.x >> 6));
        if (c < chunks) {  // (so nq >= 1)
            const uint32_t last = nq - 1u;
            uint32_t q = c * 64u + lane_id();
            uint32_t sv = gload32(qsv + min(q, last)), w = gload32(qd + min(q, last));
            uint32_t sv1 = gload32(qsv + min(q + nw * 64u, last)), w1 = gload32(qd + min(q + nw * 64u, last));
            uint32_t r0 = gload8(reg0 + sv), ww = gload32(win + w);
            // (the first chunk needs all of these at once anyway; with nothing in flight on
            // entry, the loop's wait counts are those of its own iterations, not the fewer
            // operations that follow a load on the way in from here)
            lane_drain();
            for (; c < chunks; c += nw) {
#if MR_LANE_QUERY_DEPTH == 1
                const uint32_t q1 = min(q + nw * 64u, last);
                sv1 = gload32(qsv + q1), w1 = gload32(qd + q1);
#else
                const uint32_t q2 = min(q + 2u * nw * 64u, last);
                const uint32_t sv2 = gload32(qsv + q2), w2 = gload32(qd + q2);
#endif
                const uint32_t r1 = gload8(reg0 + sv1), ww1 = gload32(win + w1);
#ifdef MR_STAMPS
                // (diagnostic builds wait here for the chunk's own gathers, to time the wait)
                asm volatile("" ::"v"(r0), "v"(ww));
                {
                    const unsigned long long now_ = __builtin_amdgcn_s_memtime();
                    H.lst[1] += now_ - H.lst_last;  // (1 in this mode: the loads and the wait for them)
                    H.lst_last = now_;
                }
#endif
                written += H.query_record(q < nq, q, c * 64u, sv, w, r0, ww, rows);
                q += nw * 64u;
                sv = sv1, w = w1, r0 = r1, ww = ww1;
#if MR_LANE_QUERY_DEPTH != 1
                sv1 = sv2, w1 = w2;
#endif
            }
        }
    } else if constexpr (MODE == kLaneStage) {  // whole waves: the rows' stores are the wave's
        H.STW = smem + lane_memo_lds_bytes(NS, nreg, TM) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kLaneStageWave;
        const uint32_t n = a->n_lane;
        const bool have = s_idx < n;
        if (__any(have)) written = H.memo_solve(have ? s_idx : n - 1u, rows, have);
    } else {
        if (s_idx < a->n_lane) written = H.memo_solve(s_idx, rows);
    }
#ifdef MR_STAMPS
    {
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();
        H.lst[5] += now_ - H.lst_last;  // (5: the source's row and the destinations)
        if (a->dbg && lane_id() == 0) {
            unsigned long long *h = a->dbg + (unsigned long long)a->dbg_blocks * 10 + 9;
            atomicAdd(h, 1ull);
            for (int i = 0; i < 6; ++i) atomicAdd(h + 1 + i, H.lst[i]);
            atomicAdd(h - 2, H.lst[6]);
        }
    }
#endif
    __shared__ uint32_t wsum;
    if (threadIdx.x == 0) wsum = 0;
    __syncthreads();
    if (written) atomicAdd(&wsum, written);
    __syncthreads();
    if (threadIdx.x == 0) finish_launch(a, wsum);
}

// The gate holds where every special is reached at 0 legs under a Legs-first order (perms
// 5 and 7).  The other orders are instantiated too, so that the gate alone decides.
#define MR_MEMO_FN(FN, ...)                                                          \
    static const void *FN(uint32_t perm) {                                           \
        switch (perm) {                                                              \
            case 5: return reinterpret_cast<const void *>(&__VA_ARGS__(5));          \
            case 7: return reinterpret_cast<const void *>(&__VA_ARGS__(7));          \
            case 11: return reinterpret_cast<const void *>(&__VA_ARGS__(11));        \
            case 15: return reinterpret_cast<const void *>(&__VA_ARGS__(15));        \
            case 19: return reinterpret_cast<const void *>(&__VA_ARGS__(19));        \
            case 21: return reinterpret_cast<const void *>(&__VA_ARGS__(21));        \
            default: return nullptr;                                                 \
        }                                                                            \
    }
#define MR_K_BUILD(P) hub_lane_build_kernel<P, 22>
#define MR_K_MEMO(P) hub_lane_memo_kernel<P, 22, kLaneMemo>
#define MR_K_READ(P) hub_lane_memo_kernel<P, 22, kLaneWin>
#define MR_K_WIN(P) hub_lane_win_kernel<P, 22>
#define MR_K_STAGE(P) hub_lane_memo_kernel<P, 22, kLaneStage>
#define MR_K_QUERY(P) hub_lane_memo_kernel<P, 22, kLaneQuery>
MR_MEMO_FN(hub_lane_build_kernel_fn, MR_K_BUILD)
MR_MEMO_FN(hub_lane_memo_kernel_fn, MR_K_MEMO)
MR_MEMO_FN(hub_lane_read_kernel_fn, MR_K_READ)
MR_MEMO_FN(hub_lane_win_kernel_fn, MR_K_WIN)
MR_MEMO_FN(hub_lane_stage_kernel_fn, MR_K_STAGE)
MR_MEMO_FN(hub_lane_query_kernel_fn, MR_K_QUERY)
#undef MR_K_BUILD
#undef MR_K_MEMO
#undef MR_K_READ
#undef MR_K_WIN
#undef MR_K_STAGE
#undef MR_K_QUERY
#undef MR_MEMO_FN

uint32_t hub_lane_lds_bytes(uint32_t NS, uint32_t nreg);

// words of one memo row and rows of a plan (22-entry tables only)
uint32_t lane_memo_words(uint32_t NS, uint32_t nreg) { return (nreg + NS) * lane_memo_row_words(22); }

// d_args: the plan's arguments with src_v = the rows' sources (nreg region
// representatives, then the NS specials' cells), n_lane = nreg + NS, lane_memo = the rows
hipError_t launch_lane_memo_build(const KArgs *d_args, const uint32_t perm[3], uint32_t NS, uint32_t nreg,
                                  hipStream_t stream) {
    if (NS + 1 > 22 || nreg + NS > 64) return hipErrorInvalidValue;
    const void *fn = hub_lane_build_kernel_fn(perm[0] * 9 + perm[1] * 3 + perm[2]);
    if (!fn) return hipErrorInvalidValue;
    const uint32_t bytes = hub_lane_lds_bytes(NS, nreg);
    if (bytes > 64u * 1024u) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
    void *args[] = {const_cast<KArgs **>(&d_args)};
    return hipLaunchKernel(fn, dim3(1), dim3(kBS), args, bytes, stream);
}

// d_args: launch_lane_memo_build's arguments with the rows built, lane_win = V words and
// lane_reg0 = V bytes to fill
hipError_t launch_lane_win_build(const KArgs *d_args, const uint32_t perm[3], uint32_t NS, uint32_t nreg, uint32_t V,
                                 hipStream_t stream) {
    const void *fn = hub_lane_win_kernel_fn(perm[0] * 9 + perm[1] * 3 + perm[2]);
    if (!fn || NS + 1 > 22 || nreg > kLaneRegs || !V) return hipErrorInvalidValue;
    void *args[] = {const_cast<KArgs **>(&d_args)};
    return hipLaunchKernel(fn, dim3((V + kBS - 1u) / kBS), dim3(kBS), args, lane_memo_lds_bytes(NS, nreg, 22), stream);
}

// the widest plan (command slots a record) the staged kernel takes
uint32_t lane_stage_max_cmds() { return kLaneStageSlots; }

// win: the arguments hold the winner table (lane_win, lane_reg0); stage: and the command
// rows leave through the stage (max_cmds 1 .. lane_stage_max_cmds()).  lds_pad: bytes of
// LDS the kernel does not use, which hold it to fewer workgroups a CU (occupancy scans)
hipError_t launch_hub_lane_memo(const KArgs *d_args, const uint32_t perm[3], uint32_t NS, uint32_t nreg, uint32_t n_lane,
                                bool win, bool stage, uint32_t lds_pad, hipStream_t stream, const hipEvent_t *timed) {
    const uint32_t pi = perm[0] * 9 + perm[1] * 3 + perm[2];
    const void *fn = stage ? hub_lane_stage_kernel_fn(pi) : win ? hub_lane_read_kernel_fn(pi) : hub_lane_memo_kernel_fn(pi);
    if (!fn || NS + 1 > 22 || (stage && !win)) return hipErrorInvalidValue;
    const uint32_t bytes = (stage ? lane_stage_lds_bytes(NS, nreg, 22) : lane_memo_lds_bytes(NS, nreg, 22)) + lds_pad;
    if (bytes > 64u * 1024u) return hipErrorInvalidValue;
    const uint32_t waves = (n_lane + 63u) / 64u, blocks = (waves + 3u) / 4u;
    void *args[] = {const_cast<KArgs **>(&d_args)};
    return launch_pass(fn, dim3(blocks ? blocks : 1u), dim3(kBS), args, bytes, stream, timed);
}

// KArgs::q_srcv of a plan: a thread per lane source writes its cell over its records
__global__ __launch_bounds__(kBS) void lane_query_expand_kernel(const uint32_t *__restrict__ src_v,
                                                                const uint32_t *__restrict__ q_begin, uint32_t n_lane,
                                                                uint32_t *__restrict__ q_srcv) {
    const uint32_t s = blockIdx.x * kBS + threadIdx.x;
    if (s >= n_lane) return;
    const uint32_t v = src_v[s], qb = q_begin[s + 1];
    for (uint32_t q = q_begin[s]; q < qb; ++q) q_srcv[q] = v;
}
hipError_t launch_lane_query_expand(const uint32_t *src_v, const uint32_t *q_begin, uint32_t n_lane, uint32_t *q_srcv,
                                    hipStream_t stream) {
    if (!n_lane) return hipSuccess;
    hipLaunchKernelGGL(lane_query_expand_kernel, dim3((n_lane + kBS - 1u) / kBS), dim3(kBS), 0, stream, src_v, q_begin,
                       n_lane, q_srcv);
    return hipGetLastError();
}

// the workgroups of `fn` with `bytes` of LDS that the device holds at once (asked once per
// (device, function, LDS size)); 0: the query failed
static uint32_t resident_workgroups(const void *fn, uint32_t bytes) {
    static std::mutex mu;
    static std::map<std::tuple<int, const void *, uint32_t>, uint32_t> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(dev, fn, bytes);
    const auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, int(kBS), bytes) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 || cus < 1) {
        (void)hipGetLastError();
        return 0;
    }
    return cache[key] = uint32_t(per_cu) * uint32_t(cus);
}

// hub_lane_memo_kernel<.., kLaneQuery> over the nq_lane records of the lane sources (d_args:
// the winner table, q_srcv and nq_lane set): min(a workgroup per 256 records, the resident
// workgroups), each wave walking chunks of 64 records at the grid's stride.  grid_cap
// (diagnostic, MR_LANE_QUERY_GRID): at most this many workgroups, 0: no cap; kNone32: a
// workgroup per 256 records whatever is resident (every wave takes one chunk)
hipError_t launch_hub_lane_query(const KArgs *d_args, const uint32_t perm[3], uint32_t NS, uint32_t nreg, uint32_t nq_lane,
                                 uint32_t grid_cap, uint32_t lds_pad, hipStream_t stream, const hipEvent_t *timed) {
    const void *fn = hub_lane_query_kernel_fn(perm[0] * 9 + perm[1] * 3 + perm[2]);
    if (!fn || NS + 1 > 22) return hipErrorInvalidValue;
    const uint32_t bytes = lane_memo_lds_bytes(NS, nreg, 22) + lds_pad;
    if (bytes > 64u * 1024u) return hipErrorInvalidValue;
    uint32_t blocks = std::max(1u, (nq_lane + kBS - 1u) / kBS);
    if (grid_cap != kNone32) {
        const uint32_t res = resident_workgroups(fn, bytes);
        if (!res) return hipErrorInvalidValue;
        blocks = std::min(blocks, res);
        if (grid_cap) {
            blocks = std::min(blocks, grid_cap);
        } else {
            // The waves take the chunks in rounds, and a round costs about the same
            // whether its last waves have a chunk or not: the fewest workgroups that keep
            // the round count, so that the last round is as full as the others (c4: 15 625
            // chunks, 1 024 resident workgroups: 4 rounds either way, of 977 workgroups)
            const uint32_t chunks = (nq_lane + 63u) / 64u, wpb = kBS / 64u;
            const uint32_t rounds = (chunks + blocks * wpb - 1u) / (blocks * wpb);
            blocks = std::max(1u, (chunks + rounds * wpb - 1u) / (rounds * wpb));
        }
    }
    void *args[] = {const_cast<KArgs **>(&d_args)};
    return launch_pass(fn, dim3(blocks), dim3(kBS), args, bytes, stream, timed);
}

}  // namespace mr
