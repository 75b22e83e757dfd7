// mr_nearest.hpp — nearest plans: per source and destination group, the best listed
// destination's record and which destination it was (DESIGN.md section 3b'').
//
// The per-source set-up and the per-destination evaluation are matrix_kernel's (mr_matrix.hpp),
// copied and not shared, so that kernel's code and registers stay what they were: a lane
// evaluates one destination to its cell word and expands it with expand_word, so the record of a
// winner equals its matrix record word for word.  What is new is the reduction.  The
// destinations arrive stable-sorted by group and cut into chunks of at most 64 that never span
// two groups (KArgs::nr_chunk).  A lane's key is (o[q0], o[q1], o[q2], sorted index); each lane
// keeps the least key of the destinations it has met in the current group (three compares a
// chunk, no cross-lane traffic), and when the group ends the wave narrows the lanes' keys word by
// word on the DPP network (four wave_min_u32).  The sort is stable, so the smallest sorted index
// of a group is the caller's smallest position.  The winning lane stores the 32 B record with
// the caller's position (KArgs::nr_pos).
//
// A group's chunks stay in one wave: no cross-wave combine, no atomics, no second launch.  With
// fewer sources than waves, the waves that share a source split its groups into contiguous
// ranges; with many sources a wave takes whole sources.  One source with one huge group is
// therefore one wave's work (the documented bad case).
#pragma once
#include "mr_device.hpp"

namespace mr {

// the 32 B record of group g (two 16 B stores of one lane); pos = all ones and the other words 0:
// an empty group
__device__ __forceinline__ void nearest_store(uint4 *row, uint32_t g, uint32_t legs, uint32_t money, uint32_t time_s,
                                              uint32_t via, uint32_t pos) {
    row[2ull * g] = make_uint4(legs, money, time_s, via);
    row[2ull * g + 1] = make_uint4(pos, 0u, 0u, 0u);
}

template <uint32_t PERM>
__global__ __launch_bounds__(kBS) void nearest_kernel(const KArgs *__restrict__ a) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    // per unit of walk distance: legs 1, money 0, time 180 s
    constexpr uint32_t sl[3] = {1u, 0u, 180u};
    // per wave: matrix_kernel's tables (boundaries by rank, the cell word's table index, the
    // packed key, the lead's base; by table index the entries' metrics)
    __shared__ uint32_t btab[kBS / 64][11][64];
    const uint32_t lane = threadIdx.x & 63u, wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t(*B)[64] = btab[wv];
    uint32_t(*M)[64] = btab[wv] + 8;
    const uint32_t NS = a->p.NS, T = NS + 1, S = a->p.S, nsrc = a->nsrc;
    const uint32_t ng = a->nr_ngroups, pitch = a->mx_pitch;
    const uint32_t fn = a->p.ff_num, fd = a->p.ff_den;
    const FfRatio ff{fn, fd};
    const bool nonlin = fn != fd;
    const int H = int(a->p.H);
    const bool no_pack = (a->dbg_flags & 2u) != 0;
    const uint32_t nwaves = gridDim.x * (kBS / 64), gw = blockIdx.x * (kBS / 64) + wv;
    // waves that share a source: none when the sources fill the waves, else they split its groups
    const uint32_t nshare = max(1u, min(nsrc, nwaves)), G = nwaves / nshare, g = gw / G, j = gw % G;
    const uint2 *const dst = a->mx_dst;
    const uint4 *const chunk = a->nr_chunk;
    // this wave's groups [g0, g1) of every source it takes, and their chunks [cb, ce)
    const uint32_t g0 = uint32_t((unsigned long long)ng * j / G), g1 = uint32_t((unsigned long long)ng * (j + 1) / G);
    const uint32_t cb = g0 < g1 ? a->nr_gstart[g0] : 0u, ce = g0 < g1 ? a->nr_gstart[g1] : 0u;
    for (uint32_t s = g; g < nshare && g0 < g1 && s < nsrc; s += nshare) {
        if (a->src_state[s] != 1) continue;  // solved by the SSSP kernel, which wrote its records
        // the first chunk and its destinations, ahead of the tables' loads
        uint4 chn = make_uint4(0u, 0u, 0u, 0u);
        uint2 dn = make_uint2(0u, 0u);
        if (cb < ce) {
            chn = chunk[cb];
            if (lane < chn.z) dn = dst[chn.y + lane];
        }
        // ---- this source's tables (matrix_kernel's, "this source's tables") ----------------
        const unsigned long long tb = (unsigned long long)s * T;
        const uint32_t src = a->src_v[s];
        const int sx = int(src % S) - H, sy = int(src / S) - H;
        wave_sync();  // the previous source's tables have been read
        uint32_t r = kNone32, e0 = 0, e1 = 0, e2 = 0;
        if (lane < T) {
            r = a->out_lex[tb + lane];
            const Rec &e = a->out_tab[tb + lane];
            e0 = e.m[0];
            e1 = e.m[1];
            e2 = e.m[2];
            M[0][lane] = e0;
            M[1][lane] = e1;
            M[2][lane] = e2;
            if (r != kNone32) {
                B[0][r] = lane == 0 ? uint32_t(sx) : uint32_t(a->sp[lane].x);
                B[1][r] = lane == 0 ? uint32_t(sy) : uint32_t(a->sp[lane].y);
                B[2][r] = e0;
                B[3][r] = e1;
                B[4][r] = e2;
            }
        }
        const bool isb = lane < T && r != kNone32;
        const uint32_t nb = uint32_t(__popcll(__ballot(isb)));
        const uint64_t dmax = 2ull * S + 2;  // the longest walk (round the Center)
        const uint64_t em[3] = {e0, e1, e2};
        // the lead metric, the kept set (Money first) and the tie order srank: see fill_body
        constexpr uint32_t L = q0 == 1 ? q1 : q0, T1 = q0 == 1 ? q2 : q1, T2 = q0 == 1 ? 3u : q2;
        constexpr uint32_t sL = sl[L];
        bool kept = isb;
        if (q0 == 1) {
            uint32_t mmin = isb ? e1 : 0xFFFFFFFFu;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mmin = min(mmin, uint32_t(__shfl_xor(int(mmin), o)));
            kept = isb && e1 == mmin;
        }
        const unsigned long long keptm = __ballot(kept);
        const uint32_t nk = uint32_t(__popcll(keptm));
        uint32_t srank = 0;
        const long long c1 = (long long)sL * (long long)em[T1] - (long long)sl[T1] * (long long)em[L];
        const long long c2 = T2 < 3u ? (long long)sL * (long long)em[T2 % 3u] - (long long)sl[T2 % 3u] * (long long)em[L] : 0;
        for (unsigned long long m = keptm; m; m &= m - 1) {
            const int o = __ffsll((long long)m) - 1;  // table index of a kept boundary
            const uint32_t ro = uint32_t(__shfl(int(r), o));
            const long long o1 = __shfl(c1, o), o2 = __shfl(c2, o);
            srank += (o1 < c1 || (o1 == c1 && (o2 < c2 || (o2 == c2 && ro < r)))) ? 1u : 0u;
        }
        uint64_t mxL = kept ? em[L] + sL * dmax : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mxL = max(mxL, (uint64_t)__shfl_xor((unsigned long long)mxL, o));
        const uint32_t rbs = max(1u, bit_width64(nk - 1));
        const uint32_t wL = uint32_t(__builtin_amdgcn_readfirstlane(int(max(1u, bit_width64(mxL)))));
        // keys wider than 32 bits (or MR_DBG_FLAGS bit 1): the full compare
        const bool packable = !no_pack && !nonlin && wL + rbs <= 32u;
        const uint32_t stepL = packable ? sL << rbs : 0u, maskr = (1u << rbs) - 1u;
        if (packable) {
            if (isb) B[6][r] = kept ? uint32_t(em[L] << rbs) | srank : 0xFFFFFFFFu;  // by rank
            if (kept) {  // by srank: the cell word's table index and the lead's base
                B[5][srank] = lane;
                B[7][srank] = uint32_t(em[L]);
            }
        } else if (isb) {
            B[5][r] = lane;  // by rank
        }
        wave_sync();
        // rank `lane`'s boundary in registers: the boundary loop reads them with v_readlane
        const uint32_t bx_l = lane < nb ? B[0][lane] : 0u, by_l = lane < nb ? B[1][lane] : 0u;
        const uint32_t bk_l = lane < nb && packable ? B[6][lane] : 0u;
        const unsigned long long live = __ballot(lane < nb && (!packable || bk_l != 0xFFFFFFFFu));
        constexpr uint32_t kBias = 0x8000u;
        const uint32_t bxu_l = bx_l + kBias, byu_l = by_l + kBias;
        const unsigned long long axm = __ballot(lane < nb && (bx_l == 0u || by_l == 0u)) & live;
        // ---- this wave's groups of the source's row --------------------------------------
        uint4 *const row = a->mx_rows + 2ull * (unsigned long long)s * pitch;
        // The running best of group `cur`, per lane: the least key among the destinations this
        // lane has evaluated for the group (metrics in comparator order, the sorted index; all
        // ones: none yet) and that destination's via.  A lane meets its destinations in sorted
        // order, so a strict compare of the metrics keeps the earliest of equals.  The wave is
        // reduced once a group, when it ends: narrowed word by word on the DPP network (four
        // wave_min_u32), the sorted index last, which is unique.
        uint32_t cur = g0, b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu, b3 = 0xFFFFFFFFu, bvia = 0u;
        const auto flush = [&](uint32_t upto) {  // the records of groups [cur, upto): cur's best, then empty ones
            bool cand = b3 != 0xFFFFFFFFu;
            if (__ballot(cand) != 0) {
                const uint32_t m0 = wave_min_u32(cand ? b0 : 0xFFFFFFFFu);
                cand = cand && b0 == m0;
                const uint32_t m1 = wave_min_u32(cand ? b1 : 0xFFFFFFFFu);
                cand = cand && b1 == m1;
                const uint32_t m2 = wave_min_u32(cand ? b2 : 0xFFFFFFFFu);
                cand = cand && b2 == m2;
                const uint32_t m3 = wave_min_u32(cand ? b3 : 0xFFFFFFFFu);
                if (cand && b3 == m3) {  // one lane: the winner's
                    const uint32_t k[3] = {m0, m1, m2};
                    // (metric m is key word i where q_i == m)
                    const uint32_t legs = k[q0 == 0 ? 0 : (q1 == 0 ? 1 : 2)], money = k[q0 == 1 ? 0 : (q1 == 1 ? 1 : 2)];
                    const uint32_t time_s = k[q0 == 2 ? 0 : (q1 == 2 ? 1 : 2)];
                    nearest_store(row, cur, legs, money, time_s, bvia, a->nr_pos[m3]);
                }
                b0 = b1 = b2 = b3 = 0xFFFFFFFFu;
                ++cur;
            }
            for (; cur < upto; ++cur)
                if (lane == 0) nearest_store(row, cur, 0u, 0u, 0u, 0u, 0xFFFFFFFFu);
        };
        for (uint32_t c = cb; c < ce; ++c) {
            const uint4 ch = chn;
            const uint2 d = dn;
            // the next chunk and its destinations before this chunk's work and stores (vmcnt
            // counts stores too: a load issued after them would wait for them)
            chn = make_uint4(0u, 0u, 0u, 0u);
            dn = make_uint2(0u, 0u);
            if (c + 1 < ce) {
                chn = chunk[c + 1];
                if (lane < chn.z) dn = dst[chn.y + lane];
            }
            const uint32_t cg = uint32_t(__builtin_amdgcn_readfirstlane(int(ch.x)));
            const uint32_t cfirst = uint32_t(__builtin_amdgcn_readfirstlane(int(ch.y)));
            const uint32_t ccount = uint32_t(__builtin_amdgcn_readfirstlane(int(ch.z)));
            if (cg != cur) flush(cg);
            const int x = int(short(d.x & 0xFFFFu)), y = int(short(d.x >> 16));
            CellWord w;
            if (packable) {
                uint32_t key = 0xFFFFFFFFu;
                const uint32_t xu = uint32_t(x) + kBias, yu = uint32_t(y) + kBias;
                for (unsigned long long m = live & ~axm; m; m &= m - 1) {  // the kept boundaries off the axes
                    const uint32_t rr = uint32_t(__ffsll((long long)m) - 1);
                    const uint32_t bxu = uint32_t(__builtin_amdgcn_readlane(int(bxu_l), int(rr)));
                    const uint32_t byu = uint32_t(__builtin_amdgcn_readlane(int(byu_l), int(rr)));
                    const uint32_t K = uint32_t(__builtin_amdgcn_readlane(int(bk_l), int(rr)));
                    key = min(key, K + __umul24(stepL, __usad(yu, byu, __usad(xu, bxu, 0u))));
                }
                if (axm) {
                    // this cell's detour from a boundary on its axis on the other side of the Center
                    const uint32_t dxn = y == 0 && x < 0 ? 2u : 0u, dxp = y == 0 && x > 0 ? 2u : 0u;
                    const uint32_t dyn = x == 0 && y < 0 ? 2u : 0u, dyp = x == 0 && y > 0 ? 2u : 0u;
                    for (unsigned long long m = axm; m; m &= m - 1) {
                        const uint32_t rr = uint32_t(__ffsll((long long)m) - 1);
                        const int bx = __builtin_amdgcn_readlane(int(bx_l), int(rr));
                        const int by = __builtin_amdgcn_readlane(int(by_l), int(rr));
                        const uint32_t K = uint32_t(__builtin_amdgcn_readlane(int(bk_l), int(rr)));
                        uint32_t det = 0u;  // (bx, by wave-uniform: the branches are scalar)
                        if (by == 0 && bx != 0) det = bx < 0 ? dxp : dxn;
                        else if (bx == 0 && by != 0) det = by < 0 ? dyp : dyn;
                        const uint32_t dd = __usad(yu, uint32_t(by) + kBias, __usad(xu, uint32_t(bx) + kBias, 0u)) + det;
                        key = min(key, K + __umul24(stepL, dd));
                    }
                }
                // the cell word b << 20 | k: k = (lead - the boundary's lead) / sL
                const uint32_t sr = key & maskr, lead = key >> rbs;
                const uint32_t k = sL == 1u ? lead - B[7][sr] : (lead - B[7][sr]) / sL;
                w = (B[5][sr] << kStBShift) | k;
            } else {
                // the three-metric compare of fill_tile_rows: rank order, the first of equal
                // metrics wins
                uint32_t r0 = 0xFFFFFFFFu, r1 = 0xFFFFFFFFu, r2 = 0xFFFFFFFFu, rb = 0u, rk = 0u;
                for (uint32_t rr = 0; rr < nb; ++rr) {
                    const uint32_t dd = walk_dist(int(B[0][rr]), int(B[1][rr]), x, y);
                    const uint32_t t0 = B[2][rr], t1 = B[3][rr], t2 = B[4][rr];
                    const uint32_t mm0 = t0 + dd, mm2 = t2 + run_time_ff(dd, fn, fd);
                    const uint32_t n1 = q0 == 0 ? mm0 : (q0 == 1 ? t1 : mm2);
                    const uint32_t n2 = q1 == 0 ? mm0 : (q1 == 1 ? t1 : mm2);
                    const uint32_t n3 = q2 == 0 ? mm0 : (q2 == 1 ? t1 : mm2);
                    const uint32_t k1 = q0 == 0 ? r0 : (q0 == 1 ? r1 : r2);
                    const uint32_t k2 = q1 == 0 ? r0 : (q1 == 1 ? r1 : r2);
                    const uint32_t k3 = q2 == 0 ? r0 : (q2 == 1 ? r1 : r2);
                    const bool better = n1 < k1 || (n1 == k1 && (n2 < k2 || (n2 == k2 && n3 < k3)));
                    r0 = better ? mm0 : r0;
                    r1 = better ? t1 : r1;
                    r2 = better ? mm2 : r2;
                    rb = better ? B[5][rr] : rb;
                    rk = better ? dd : rk;
                }
                w = (rb << kStBShift) | rk;
            }
            // specials hold their own labels, the source's cell (it may also be a special) the
            // start label
            if (d.y & kViaSpecial) w = d.y;
            if (x == sx && y == sy) w = kViaSource;
            mr_label_record o{0u, 0u, 0u, 0u};
            const bool cand = lane < ccount;
            if (cand && !expand_word(w, T, ff, [&](uint32_t t, uint32_t q) { return M[q][t]; }, o))
                atomicOr(a->counter + kCtrFlags, kErrChain);
            // ---- this lane's running best: (o[q0], o[q1], o[q2]) strictly below it ----
            const uint32_t om[3] = {o.legs, o.money, o.time_s};
            const uint32_t n0 = om[q0], n1 = om[q1], n2 = om[q2];
            const bool better = cand && (b3 == 0xFFFFFFFFu || n0 < b0 || (n0 == b0 && (n1 < b1 || (n1 == b1 && n2 < b2))));
            b0 = better ? n0 : b0;
            b1 = better ? n1 : b1;
            b2 = better ? n2 : b2;
            b3 = better ? cfirst + lane : b3;
            bvia = better ? o.via : bvia;
        }
        flush(g1);
        // pad records of the row: zeros, so rows are whole lines (the wave with the last groups)
        if (g1 == ng && lane < 2u * (pitch - ng)) row[2ull * ng + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (threadIdx.x == 0) finish_launch(a, 0);
}

}  // namespace mr
