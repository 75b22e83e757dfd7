// mr_matrix.hpp — matrix plans: the labels of listed destinations only (DESIGN.md section 3b').
//
// The hub kernel's export leaves each source's label table (out_tab) and its boundaries'
// ranks (out_lex).  The label of a plain cell is then the best walk from a boundary —
// metrics in comparator order, then the boundary's rank — exactly as the all-destinations
// fill evaluates it per tile (fill_body, mr_device.hpp).  Here one lane is one destination:
// a wave takes 64-destination chunks of one source, evaluates the closed form for its lane's
// cell and stores the expanded 16 B record {legs, money, time, via}.  Nothing is read of the
// other cells of the grid and no cell words are written.
//
// Waves form groups over the sources as in the fill (at least four waves a source when
// sources are few, the groups stride over the sources); a wave loads its source's tables
// into its own LDS slot once per source; no workgroup barriers but the one before the
// end-of-launch bookkeeping.
#pragma once
#include "mr_device.hpp"

namespace mr {

template <uint32_t PERM>
__global__ __launch_bounds__(kBS) void matrix_kernel(const KArgs *__restrict__ a) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    // per unit of walk distance: legs 1, money 0, time 180 s
    constexpr uint32_t sl[3] = {1u, 0u, 180u};
    // per wave: boundaries by rank (x, y, m0, m1, m2), the cell word's table index by srank
    // (by rank for the full compare), the packed key by rank, the lead's base by srank; and by
    // table index the entries' metrics (a special's own label, a walk's base)
    __shared__ uint32_t btab[kBS / 64][11][64];
    const uint32_t lane = threadIdx.x & 63u, wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t(*B)[64] = btab[wv];
    uint32_t(*M)[64] = btab[wv] + 8;
    const uint32_t NS = a->p.NS, T = NS + 1, S = a->p.S, nsrc = a->nsrc;
    const uint32_t ndst = a->mx_ndst, pitch = a->mx_pitch, nchunk = (pitch + 63u) / 64u;
    const uint32_t fn = a->p.ff_num, fd = a->p.ff_den;
    const FfRatio ff{fn, fd};
    const bool nonlin = fn != fd;
    const int H = int(a->p.H);
    const bool no_pack = (a->dbg_flags & 2u) != 0;
    const uint32_t nwaves = gridDim.x * (kBS / 64), gw = blockIdx.x * (kBS / 64) + wv;
    constexpr uint32_t kMinG = 4;  // waves that share a source (fill_body: kFillMinG)
    const uint32_t ngroups = max(1u, min(nsrc, max(1u, nwaves / kMinG))), G = nwaves / ngroups, g = gw / G, j = gw % G;
    const uint2 *const dst = a->mx_dst;
    for (uint32_t s = g; g < ngroups && s < nsrc; s += ngroups) {
        if (a->src_state[s] != 1) continue;  // solved by the SSSP kernel, which wrote its records
        // the first chunk's destinations, ahead of the tables' loads
        uint32_t c = j;
        uint2 dn = make_uint2(0u, 0u);
        if (c < nchunk && c * 64u + lane < ndst) dn = dst[c * 64u + lane];
        // ---- this source's tables (fill_body's, "this source's tables") ----------------
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
        // Packed keys: the walk distance as two v_sad_u32 over coordinates biased to unsigned.
        // Only a boundary on an axis through the Center can take walk_dist's 2-cell detour (to
        // cells on the same axis across the Center): those get a loop of their own, as in the fill.
        constexpr uint32_t kBias = 0x8000u;
        const uint32_t bxu_l = bx_l + kBias, byu_l = by_l + kBias;
        const unsigned long long axm = __ballot(lane < nb && (bx_l == 0u || by_l == 0u)) & live;
        // ---- this wave's chunks of the source's row -------------------------------------
        uint4 *const row = a->mx_rows + (unsigned long long)s * pitch;
        for (; c < nchunk; c += G) {
            const uint2 d = dn;
            const uint32_t jd = c * 64u + lane;
            // the next chunk's destinations before this chunk's stores (vmcnt counts stores
            // too: a load issued after them would wait for them)
            const uint32_t cn = c + G;
            dn = make_uint2(0u, 0u);
            if (cn < nchunk && cn * 64u + lane < ndst) dn = dst[cn * 64u + lane];
            const int x = int(short(d.x & 0xFFFFu)), y = int(short(d.x >> 16));
            CellWord w;
            if (packable) {
                // (keys are distinct: srank in the low bits, so the order of the minimum is free;
                // stepL and the distance fit 24 bits: sL <= 180, rbs <= 6, d <= 2 S + 2)
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
                    const uint32_t b0 = B[2][rr], b1 = B[3][rr], b2 = B[4][rr];
                    const uint32_t mm0 = b0 + dd, mm2 = b2 + run_time_ff(dd, fn, fd);
                    const uint32_t n1 = q0 == 0 ? mm0 : (q0 == 1 ? b1 : mm2);
                    const uint32_t n2 = q1 == 0 ? mm0 : (q1 == 1 ? b1 : mm2);
                    const uint32_t n3 = q2 == 0 ? mm0 : (q2 == 1 ? b1 : mm2);
                    const uint32_t k1 = q0 == 0 ? r0 : (q0 == 1 ? r1 : r2);
                    const uint32_t k2 = q1 == 0 ? r0 : (q1 == 1 ? r1 : r2);
                    const uint32_t k3 = q2 == 0 ? r0 : (q2 == 1 ? r1 : r2);
                    const bool better = n1 < k1 || (n1 == k1 && (n2 < k2 || (n2 == k2 && n3 < k3)));
                    r0 = better ? mm0 : r0;
                    r1 = better ? b1 : r1;
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
            // (a word that names no table entry: the flag write_matrix raises for it)
            if (jd < ndst && !expand_word(w, T, ff, [&](uint32_t t, uint32_t q) { return M[q][t]; }, o))
                atomicOr(a->counter + kCtrFlags, kErrChain);
            // one 16 B store a lane; rows start on a 128 B line and the pitch is whole lines,
            // so a chunk's stores are whole lines (pad records: zeros)
            if (jd < pitch) row[jd] = make_uint4(o.legs, o.money, o.time_s, o.via);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) finish_launch(a, 0);
}

}  // namespace mr
