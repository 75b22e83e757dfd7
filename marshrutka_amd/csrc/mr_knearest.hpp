// mr_knearest.hpp — k-nearest plans: per source and destination group, the records of the k
// best listed destinations in order (DESIGN.md section 3b''').
//
// Rank r of group g is the r-th least destination of the group under the nearest plan's order
// (o[q0], o[q1], o[q2], sorted index): rank 0 is nearest_kernel's winner word for word, a cell
// listed twice takes two ranks (the earlier listing first), a rank at or past the group's size
// is the empty record.  Record (g, r) sits at g * k + r of the source's row.
//
// The per-source set-up and the per-destination evaluation are nearest_kernel's
// (mr_nearest.hpp), here as helpers (kn_setup, kn_eval) that only this kernel uses: fill_body,
// matrix_kernel and nearest_kernel keep their own copies and so their code and registers.  The
// work split is nearest_kernel's too: a group's chunks stay in one wave, waves that share a
// source split its groups, no cross-wave combine, no atomics, no second launch; one source with
// one huge group is one wave's work (the documented bad case).
//
// What is new is the selection (klist_chunk, mr_device.hpp).  The wave keeps the group's sorted
// list one entry per lane, lane r < k entry r: four key words and via, all ones for none.  The
// threshold is entry k - 1's key, wave-uniform (v_readlane).  A chunk's lane offers its
// destination when its key is strictly below the threshold; while any lane does, the wave
// narrows to the least such key (four wave_min_u32, the sorted index last), inserts it (every
// lane whose entry is greater takes its lower neighbour's entry or the new key), strikes the
// winner from the candidates and reads the threshold again.
//
// The bound: candidates leave a chunk in ascending order, so a chunk costs at most
// min(k, count) insertions whatever order the caller listed the destinations in (a key
// inserted from this chunk is only ever followed by greater ones from it, which cannot push it
// out: after k of them the threshold is below every candidate left).
//
// At the group's end lane r < k stores record g * k + r (two 16 B stores; four lanes fill a
// 128 B line when k is a multiple of 4), the position from KArgs::nr_pos.
#pragma once
#include "mr_device.hpp"

namespace mr {

// what kn_setup leaves for kn_eval: the source, its boundaries by rank in registers (the
// boundary loop reads them with v_readlane) and the packed key's shape
struct KnSource {
    int sx, sy;
    uint32_t nb;       // boundaries
    bool packable;     // the packed key fits 32 bits (and MR_DBG_FLAGS bit 1 is clear)
    uint32_t stepL, maskr, rbs;
    uint32_t bx_l, by_l, bk_l, bxu_l, byu_l;
    unsigned long long live, axm;
};

constexpr uint32_t kKnBias = 0x8000u;

// this source's tables in the wave's LDS (nearest_kernel's "this source's tables"): B by rank
// (boundary position and metrics, the cell word's table index, the packed key, the lead's
// base), M by table index (the entries' metrics)
template <uint32_t PERM>
__device__ __forceinline__ KnSource kn_setup(const KArgs *__restrict__ a, uint32_t s, uint32_t lane, uint32_t (*B)[64],
                                             uint32_t (*M)[64]) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    // per unit of walk distance: legs 1, money 0, time 180 s
    constexpr uint32_t sl[3] = {1u, 0u, 180u};
    const uint32_t NS = a->p.NS, T = NS + 1, S = a->p.S;
    const int H = int(a->p.H);
    const bool nonlin = a->p.ff_num != a->p.ff_den, no_pack = (a->dbg_flags & 2u) != 0;
    KnSource k;
    const unsigned long long tb = (unsigned long long)s * T;
    const uint32_t src = a->src_v[s];
    k.sx = int(src % S) - H;
    k.sy = int(src / S) - H;
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
            B[0][r] = lane == 0 ? uint32_t(k.sx) : uint32_t(a->sp[lane].x);
            B[1][r] = lane == 0 ? uint32_t(k.sy) : uint32_t(a->sp[lane].y);
            B[2][r] = e0;
            B[3][r] = e1;
            B[4][r] = e2;
        }
    }
    const bool isb = lane < T && r != kNone32;
    k.nb = uint32_t(__popcll(__ballot(isb)));
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
    k.rbs = max(1u, bit_width64(nk - 1));
    const uint32_t wL = uint32_t(__builtin_amdgcn_readfirstlane(int(max(1u, bit_width64(mxL)))));
    // keys wider than 32 bits (or MR_DBG_FLAGS bit 1): the full compare
    k.packable = !no_pack && !nonlin && wL + k.rbs <= 32u;
    k.stepL = k.packable ? sL << k.rbs : 0u;
    k.maskr = (1u << k.rbs) - 1u;
    if (k.packable) {
        if (isb) B[6][r] = kept ? uint32_t(em[L] << k.rbs) | srank : 0xFFFFFFFFu;  // by rank
        if (kept) {  // by srank: the cell word's table index and the lead's base
            B[5][srank] = lane;
            B[7][srank] = uint32_t(em[L]);
        }
    } else if (isb) {
        B[5][r] = lane;  // by rank
    }
    wave_sync();
    // rank `lane`'s boundary in registers
    k.bx_l = lane < k.nb ? B[0][lane] : 0u;
    k.by_l = lane < k.nb ? B[1][lane] : 0u;
    k.bk_l = lane < k.nb && k.packable ? B[6][lane] : 0u;
    k.live = __ballot(lane < k.nb && (!k.packable || k.bk_l != 0xFFFFFFFFu));
    k.bxu_l = k.bx_l + kKnBias;
    k.byu_l = k.by_l + kKnBias;
    k.axm = __ballot(lane < k.nb && (k.bx_l == 0u || k.by_l == 0u)) & k.live;
    return k;
}

// destination d = {x | y << 16, special or cell} from the source of k: its cell word (the packed
// key, the full compare, the axis-detour loop: nearest_kernel's evaluation)
template <uint32_t PERM>
__device__ __forceinline__ CellWord kn_eval(const KArgs *__restrict__ a, const KnSource &k, uint32_t (*B)[64], uint2 d) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    constexpr uint32_t sl[3] = {1u, 0u, 180u};
    constexpr uint32_t L = q0 == 1 ? q1 : q0;
    constexpr uint32_t sL = sl[L];
    const uint32_t fn = a->p.ff_num, fd = a->p.ff_den;
    const int x = int(short(d.x & 0xFFFFu)), y = int(short(d.x >> 16));
    CellWord w;
    if (k.packable) {
        uint32_t key = 0xFFFFFFFFu;
        const uint32_t xu = uint32_t(x) + kKnBias, yu = uint32_t(y) + kKnBias;
        for (unsigned long long m = k.live & ~k.axm; m; m &= m - 1) {  // the kept boundaries off the axes
            const uint32_t rr = uint32_t(__ffsll((long long)m) - 1);
            const uint32_t bxu = uint32_t(__builtin_amdgcn_readlane(int(k.bxu_l), int(rr)));
            const uint32_t byu = uint32_t(__builtin_amdgcn_readlane(int(k.byu_l), int(rr)));
            const uint32_t K = uint32_t(__builtin_amdgcn_readlane(int(k.bk_l), int(rr)));
            key = min(key, K + __umul24(k.stepL, __usad(yu, byu, __usad(xu, bxu, 0u))));
        }
        if (k.axm) {
            // this cell's detour from a boundary on its axis on the other side of the Center
            const uint32_t dxn = y == 0 && x < 0 ? 2u : 0u, dxp = y == 0 && x > 0 ? 2u : 0u;
            const uint32_t dyn = x == 0 && y < 0 ? 2u : 0u, dyp = x == 0 && y > 0 ? 2u : 0u;
            for (unsigned long long m = k.axm; m; m &= m - 1) {
                const uint32_t rr = uint32_t(__ffsll((long long)m) - 1);
                const int bx = __builtin_amdgcn_readlane(int(k.bx_l), int(rr));
                const int by = __builtin_amdgcn_readlane(int(k.by_l), int(rr));
                const uint32_t K = uint32_t(__builtin_amdgcn_readlane(int(k.bk_l), int(rr)));
                uint32_t det = 0u;  // (bx, by wave-uniform: the branches are scalar)
                if (by == 0 && bx != 0) det = bx < 0 ? dxp : dxn;
                else if (bx == 0 && by != 0) det = by < 0 ? dyp : dyn;
                const uint32_t dd = __usad(yu, uint32_t(by) + kKnBias, __usad(xu, uint32_t(bx) + kKnBias, 0u)) + det;
                key = min(key, K + __umul24(k.stepL, dd));
            }
        }
        // the cell word b << 20 | k: k = (lead - the boundary's lead) / sL
        const uint32_t sr = key & k.maskr, lead = key >> k.rbs;
        const uint32_t kk = sL == 1u ? lead - B[7][sr] : (lead - B[7][sr]) / sL;
        w = (B[5][sr] << kStBShift) | kk;
    } else {
        // the three-metric compare of fill_tile_rows: rank order, the first of equal metrics wins
        uint32_t r0 = 0xFFFFFFFFu, r1 = 0xFFFFFFFFu, r2 = 0xFFFFFFFFu, rb = 0u, rk = 0u;
        for (uint32_t rr = 0; rr < k.nb; ++rr) {
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
    // specials hold their own labels, the source's cell (it may also be a special) the start label
    if (d.y & kViaSpecial) w = d.y;
    if (x == k.sx && y == k.sy) w = kViaSource;
    return w;
}

template <uint32_t PERM>
__global__ __launch_bounds__(kBS) void knearest_kernel(const KArgs *__restrict__ a) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;  // the key's words: o[q0], o[q1], o[q2]
    // per wave: nearest_kernel's tables
    __shared__ uint32_t btab[kBS / 64][11][64];
    const uint32_t lane = threadIdx.x & 63u, wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t(*B)[64] = btab[wv];
    uint32_t(*M)[64] = btab[wv] + 8;
    const uint32_t T = a->p.NS + 1, nsrc = a->nsrc;
    const uint32_t ng = a->nr_ngroups, pitch = a->mx_pitch;
    const uint32_t k = uint32_t(__builtin_amdgcn_readfirstlane(int(a->nr_k)));
    const FfRatio ff{a->p.ff_num, a->p.ff_den};
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
        const KnSource ks = kn_setup<PERM>(a, s, lane, B, M);
        uint4 *const row = a->mx_rows + 2ull * (unsigned long long)s * pitch;
        // the sorted list of group `cur`, an entry a lane
        uint32_t cur = g0;
        KList l;
        klist_clear(l);
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
            if (cg != cur) klist_flush(row, a->nr_pos, k, cur, cg, l, q0, q1);
            const CellWord w = kn_eval<PERM>(a, ks, B, d);
            mr_label_record o{0u, 0u, 0u, 0u};
            const bool cand = lane < ccount;
            if (cand && !expand_word(w, T, ff, [&](uint32_t t, uint32_t q) { return M[q][t]; }, o))
                atomicOr(a->counter + kCtrFlags, kErrChain);
            const uint32_t om[3] = {o.legs, o.money, o.time_s};
            klist_chunk(l, k, om[q0], om[q1], om[q2], cfirst, o.via, cand);
        }
        klist_flush(row, a->nr_pos, k, cur, g1, l, q0, q1);
        // pad records of the row: zeros, so rows are whole lines (the wave with the last groups)
        if (g1 == ng && lane < 2u * (pitch - ng * k)) row[2ull * ng * k + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (threadIdx.x == 0) finish_launch(a, 0);
}

}  // namespace mr
