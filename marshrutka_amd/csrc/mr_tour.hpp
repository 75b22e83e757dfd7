// mr_tour.hpp — tour plans: the best visiting order of up to MR_TOUR_MAX_STOPS stops, reduced on
// the device from the plan's own matrix rows (DESIGN.md section 3b'''').
//
// A tour lists c cells: the start, n stops and, under MR_TOUR_TO_LAST, a fixed end.  Its legs are
// the matrix records of the ordered pairs of those cells, so everything a tour needs is in the
// rows the matrix pass has just written.  Per tour:
//
//   gather   the c x c leg records into LDS, 16 B loads of which the three metrics are kept, in
//            comparator order (word i = metric q_i), so every later compare is plain
//            lexicographic on three u32 words.  The limit gate is taken here: per metric the
//            largest leg times the tour's legs must fit 32 bits, else the record reads
//            MR_ERR_LIMIT; behind the gate every sum the DP forms fits, so it adds unchecked.
//   DP       E[S][j]: the least cost of finishing the trip from stop j with the set S of stops
//            still to visit (j not in S), by layers of |S| with a barrier between layers.  The
//            base E[0][j] is the end rule: 0 (OPEN), leg j -> start (RETURN), leg j -> end
//            (TO_LAST).  The table is indexed j << n | S.  The subsets are first listed layer by
//            layer, so a layer's items (a listed subset x a stop) are dense over the lanes and
//            every active lane's inner loop has the layer's |S| steps.
//   walk     no parent pointers: from the start, at each step the smallest position k of S
//            whose leg(cur -> k) + E[S \ k][k] is the least over S.  That least value is the
//            optimum of what remains, so the walk yields the lexicographically least of the
//            optimal orders.  One lane does it and stores the 32 B record.
//
// Two geometries, one body: a wave a tour (four tours a workgroup in flight, wave-private LDS
// slots, wave_sync and no workgroup barrier) for small n, a workgroup a tour for the others.
// Units (waves or workgroups) stride over their launch's tours; there is no dequeue.
#pragma once
#include "mr_device.hpp"

namespace mr {

// LDS words of one unit's slot for tours of at most nmax stops: the gate's three maxima (and a
// pad word), the layers' fill counters and offsets (12 words each), the subsets by layer (16 bits
// each), the (nmax + 2)^2 legs and the nmax << nmax table entries, three words each
constexpr uint32_t kTourHead = 4u + 12u + 12u;
__host__ __device__ inline uint32_t tour_slot_words(uint32_t nmax) {
    return kTourHead + ((1u << nmax) + 1u) / 2u + 3u * (nmax + 2u) * (nmax + 2u) + 3u * (nmax << nmax);
}

__device__ __forceinline__ bool tour_lt(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2) {
    return a0 < b0 || (a0 == b0 && (a1 < b1 || (a1 == b1 && a2 < b2)));
}

template <uint32_t PERM, bool WAVE>
__global__ __launch_bounds__(kBS) void tour_kernel(const TourArgs a) {
    constexpr uint32_t q0 = PERM / 9, q1 = (PERM / 3) % 3, q2 = PERM % 3;
    extern __shared__ uint32_t tour_lds[];
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const uint32_t tid = WAVE ? (threadIdx.x & 63u) : threadIdx.x, nthr = WAVE ? 64u : uint32_t(kBS);
    const uint32_t unit = WAVE ? blockIdx.x * (kBS / 64) + wv : blockIdx.x;
    const uint32_t nunits = WAVE ? gridDim.x * (kBS / 64) : gridDim.x;
    const auto sync = [] {
        if (WAVE) wave_sync();
        else __syncthreads();
    };
    uint32_t *const gate = tour_lds + (WAVE ? wv * tour_slot_words(a.nmax) : 0u);
    uint32_t *const cnt = gate + 4, *const off = cnt + 12;           // per |S|: subsets listed so far, the layer's first
    uint16_t *const sub = reinterpret_cast<uint16_t *>(gate + kTourHead);  // the subsets, layer by layer
    uint32_t *const D = gate + kTourHead + ((1u << a.nmax) + 1u) / 2u;     // leg (i, j) at 3 * (i * c + j)
    uint32_t *const E = D + 3u * (a.nmax + 2u) * (a.nmax + 2u);      // entry (S, j) at 3 * (j << n | S)
    for (uint32_t t = unit; t < a.count; t += nunits) {
        const uint4 ti = a.tours[a.first + t];  // {first cell, cells, record, 0}: uniform over the unit
        const uint32_t c = ti.y, n = a.mode == MR_TOUR_TO_LAST ? c - 2u : c - 1u;
        const uint32_t legs = a.mode == MR_TOUR_OPEN ? n : n + 1u;
        const uint32_t endc = a.mode == MR_TOUR_TO_LAST ? c - 1u : 0u;  // the cell the base legs lead to
        const uint16_t *const cells = a.cells + ti.x;
        sync();  // the previous tour's table has been read
        if (tid < 3u) gate[tid] = 0u;
        if (tid < 12u) {  // layer tid starts behind the C(n, s) subsets of the layers s below it
            uint32_t o = 0u, b = 1u;
            for (uint32_t s = 0; s < tid; ++s) {
                o += b;
                b = b * (n - s) / (s + 1u);  // (0 from s = n on)
            }
            off[tid] = o;
            cnt[tid] = 0u;
        }
        sync();
        // ---- gather, and the gate's maxima --------------------------------------------------
        uint32_t mx0 = 0u, mx1 = 0u, mx2 = 0u;
        for (uint32_t e = tid; e < c * c; e += nthr) {
            const uint32_t i = e / c, j = e - i * c;
            const uint32_t pi = cells[i], pj = cells[j];
            uint4 r = a.rows[(unsigned long long)a.row_of_point[pi] * a.pitch + pj];
            if (pi == pj) r = make_uint4(0u, 0u, 0u, 0u);  // a leg from a cell to itself
            const uint32_t m[3] = {r.x, r.y, r.z};
            D[3u * e] = m[q0];
            D[3u * e + 1u] = m[q1];
            D[3u * e + 2u] = m[q2];
            mx0 = max(mx0, m[q0]);
            mx1 = max(mx1, m[q1]);
            mx2 = max(mx2, m[q2]);
        }
        if (mx0) atomicMax(&gate[0], mx0);
        if (mx1) atomicMax(&gate[1], mx1);
        if (mx2) atomicMax(&gate[2], mx2);
        sync();
        uint4 *const rec = a.records + 2ull * ti.z;
        const unsigned long long lim = 0xFFFFFFFFull;
        if ((unsigned long long)legs * gate[0] > lim || (unsigned long long)legs * gate[1] > lim ||
            (unsigned long long)legs * gate[2] > lim) {  // (uniform: every thread reads the same maxima)
            if (tid == 0u) {
                rec[0] = make_uint4(0u, 0u, 0u, uint32_t(MR_ERR_LIMIT));
                rec[1] = make_uint4(n | legs << 8 | 0xFFFF0000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);
            }
            continue;
        }
        // ---- the subsets by layer: a layer's work is then dense over the lanes ------------------
        // (a scan of the whole table per layer would have a wave pay the inner loop wherever one
        // of its lanes holds a subset of the layer, which is nearly everywhere)
        const uint32_t full = (1u << n) - 1u;
        for (uint32_t S = tid; S <= full; S += nthr) {
            const uint32_t p = uint32_t(__popc(S));
            sub[off[p] + atomicAdd(&cnt[p], 1u)] = uint16_t(S);  // (any order within a layer)
        }
        sync();
        // ---- the table, by layers of |S| ------------------------------------------------------
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t lo = off[s], items = (off[s + 1u] - lo) * n;
            for (uint32_t w = tid; w < items; w += nthr) {
                const uint32_t i = w / n, j = w - i * n, S = sub[lo + i];
                if ((S >> j) & 1u) continue;
                const uint32_t idx = (j << n) | S;
                const uint32_t *const from = D + 3u * (1u + j) * c;  // the legs out of stop j
                uint32_t b0 = 0u, b1 = 0u, b2 = 0u;
                if (s == 0u) {
                    if (a.mode != MR_TOUR_OPEN) b0 = from[3u * endc], b1 = from[3u * endc + 1u], b2 = from[3u * endc + 2u];
                } else {
                    b0 = b1 = b2 = 0xFFFFFFFFu;
                    for (uint32_t m = S; m; m &= m - 1u) {
                        const uint32_t k = uint32_t(__ffs(int(m))) - 1u;
                        const uint32_t *const l = from + 3u * (1u + k), *const r = E + 3u * ((k << n) | (S & ~(1u << k)));
                        const uint32_t v0 = l[0] + r[0], v1 = l[1] + r[1], v2 = l[2] + r[2];
                        const bool lt = m == S || tour_lt(v0, v1, v2, b0, b1, b2);
                        b0 = lt ? v0 : b0;
                        b1 = lt ? v1 : b1;
                        b2 = lt ? v2 : b2;
                    }
                }
                E[3u * idx] = b0;
                E[3u * idx + 1u] = b1;
                E[3u * idx + 2u] = b2;
            }
            sync();
        }
        // ---- the walk and the record ----------------------------------------------------------
        if (tid == 0u) {
            uint32_t cur = 0u, S = full, t0 = 0u, t1 = 0u, t2 = 0u;
            // the first three words of the record's second half: order[] is its bytes 2..11
            uint32_t ow0 = 0xFFFFFFFFu, ow1 = 0xFFFFFFFFu, ow2 = 0xFFFFFFFFu;
            for (uint32_t r = 0; r < n; ++r) {
                const uint32_t *const from = D + 3u * cur * c;
                uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu, bk = 0u;
                for (uint32_t m = S; m; m &= m - 1u) {  // ascending k, a strict compare: the smallest of equals
                    const uint32_t k = uint32_t(__ffs(int(m))) - 1u;
                    const uint32_t *const l = from + 3u * (1u + k), *const e = E + 3u * ((k << n) | (S & ~(1u << k)));
                    const uint32_t v0 = l[0] + e[0], v1 = l[1] + e[1], v2 = l[2] + e[2];
                    const bool lt = m == S || tour_lt(v0, v1, v2, b0, b1, b2);
                    b0 = lt ? v0 : b0;
                    b1 = lt ? v1 : b1;
                    b2 = lt ? v2 : b2;
                    bk = lt ? k : bk;
                }
                const uint32_t *const l = from + 3u * (1u + bk);
                t0 += l[0], t1 += l[1], t2 += l[2];
                // order[r] is byte 2 + r of the second half
                const uint32_t byte = 2u + r, sh = 8u * (byte & 3u), keep = ~(0xFFu << sh), put = bk << sh;
                ow0 = (byte >> 2) == 0u ? (ow0 & keep) | put : ow0;
                ow1 = (byte >> 2) == 1u ? (ow1 & keep) | put : ow1;
                ow2 = (byte >> 2) == 2u ? (ow2 & keep) | put : ow2;
                cur = 1u + bk;
                S &= ~(1u << bk);
            }
            if (a.mode != MR_TOUR_OPEN) {
                const uint32_t *const l = D + 3u * (cur * c + endc);
                t0 += l[0], t1 += l[1], t2 += l[2];
            }
            const uint32_t k[3] = {t0, t1, t2};
            // (metric m is key word i where q_i == m)
            const uint32_t o_legs = k[q0 == 0 ? 0 : (q1 == 0 ? 1 : 2)], o_money = k[q0 == 1 ? 0 : (q1 == 1 ? 1 : 2)];
            const uint32_t o_time = k[q0 == 2 ? 0 : (q1 == 2 ? 1 : 2)];
            rec[0] = make_uint4(o_legs, o_money, o_time, uint32_t(MR_OK));
            rec[1] = make_uint4((ow0 & 0xFFFF0000u) | n | legs << 8, ow1, ow2, 0u);
        }
    }
}

}  // namespace mr
