// mr_label.hpp — the rules that turn a pass's compact output into labels, once, for every
// reader: the device decoder and the wire encoder (mr_k_decode.hip), the host decoders
// mr_decode_records / mr_decode_wire and the three routes of mr_plan_fetch (mr_host.cpp).
// Plain inline functions for host and device; no state.
#pragma once
#include "../../include/marshrutka_pf.h"
#include "mr_engine.hpp"

namespace mr {

// What a compact command's payload scales by (mr_engine.hpp Cmd): the caravan seconds per
// distance unit, the scroll prices and the raw Fleetfoot level.
struct CmdScale {
    uint32_t rgt, soe, shq, sfm, ff;
};

// Fleetfoot (src/skill.rs:65-71): the ratio a StandardMove run's time is scaled by; levels
// above 3 leave the time raw, as level 0 does.
struct FfRatio {
    uint32_t num, den;
};
__host__ __device__ inline FfRatio ff_ratio(uint32_t ff) {
    switch (ff) {
        case 1: return {50u, 53u};
        case 2: return {100u, 109u};
        case 3: return {25u, 28u};
        default: return {1u, 1u};
    }
}

// ---- compact records (OutResult + max_cmds OutCmd slots + the overflow pool) ----
__host__ __device__ inline int rec_status(const OutResult &o) { return int(o.ncmd_status >> 16) - 16; }
__host__ __device__ inline uint32_t rec_ncmd(const OutResult &o) { return o.ncmd_status & 0xFFFFu; }
// the commands the record adds to the output pool (a record of any other status adds none)
__host__ __device__ inline uint32_t rec_pool_cmds(const OutResult &o) {
    const int st = rec_status(o);
    return (st == MR_OK || st == int(kStatusOverflow)) ? rec_ncmd(o) : 0u;
}

// Where record o keeps its n = rec_pool_cmds(o) commands: in its mc slots, or (a long
// label) in the overflow pool of novf commands at the {kOvfTag, offset, count} its first
// slot holds.  Malformed: a tag that is none, that disagrees with the record's count or
// that points past the pool, no slot to hold a tag, or a count no slots could hold.
enum class RecSource { slots, pool, malformed };
__host__ __device__ inline RecSource rec_source(const OutResult &o, const OutCmd *slots, uint32_t mc, const OutCmd *ovf,
                                                uint64_t novf, const OutCmd *&src, uint32_t &n) {
    const int st = rec_status(o);
    n = rec_pool_cmds(o);
    src = slots;
    if (st == int(kStatusOverflow)) {
        if (!mc) return RecSource::malformed;
        const OutCmd tag = slots[0];
        if (tag.kp != kOvfTag || tag.to != n || uint64_t(tag.from) + n > novf) return RecSource::malformed;
        src = ovf + tag.from;
        return RecSource::pool;
    }
    return st == MR_OK && n > mc ? RecSource::malformed : RecSource::slots;
}

// ---- commands ----
// What compact command kp = kind << 29 | payload expands to in an mr_command: Central 10 s a
// move, a StandardMove run 180 s a leg (raw: the command carries the Fleetfoot level), a
// caravan rgt seconds and 5 or 2 money a distance unit, a scroll its price.  A kind above
// kSFm costs nothing here: whether a command's kind and cells are range-checked is the
// caller's rule (the record decoders check a command only where they write it, the fetch's
// wire decoder every command it reads).
struct CmdCost {
    uint32_t kind, legs, money, fleetfoot;
    int64_t time_s;
};
__host__ __device__ inline CmdCost cmd_cost(uint32_t kp, const CmdScale &cs) {
    const uint32_t pay = kp & 0x1FFFFFFFu;
    CmdCost c{kp >> 29, 0u, 0u, 0u, 0};
    switch (c.kind) {
        case kCentral: c.time_s = int64_t(10) * pay; break;
        case kStandard:
            c.legs = pay;
            c.time_s = int64_t(180) * pay;
            c.fleetfoot = cs.ff;
            break;
        case kCaravan:
            c.time_s = int64_t(cs.rgt) * (pay >> 1);
            c.money = (pay >> 1) * ((pay & 1u) ? 5u : 2u);
            break;
        case kSoE: c.money = cs.soe; break;
        case kSHQ: c.money = cs.shq; break;
        case kSFm: c.money = cs.sfm; break;
        default: break;
    }
    return c;
}
// What the command adds to its label's time.  A label's metrics are its commands' sums (the
// reference's TotalCost sums, src/cost.rs:299-313), except that a StandardMove run counts
// its Fleetfoot ceil, ceil(180 legs num / den), not its raw time (src/skill.rs:21-30).
__host__ __device__ inline uint64_t label_time_add(const CmdCost &c, const FfRatio &r) {
    const uint64_t t = uint64_t(c.time_s);
    return c.kind == kStandard ? (t * r.num + r.den - 1) / r.den : t;
}

// ---- cell words (mr_engine.hpp CellWord) ----
// A cell word over its source's label table of T entries: the label's metrics (the table
// label's plus the final walk's: k legs, no money, the run's Fleetfoot ceil, src/cost.rs:122-124)
// and `via`.  metric(t, q) = metric q of table entry t.  False if the word names no entry.
// One rule for mr_sssp_records on the host, the matrix kernel and the SSSP kernel's matrix rows.
template <class Metric>
__host__ __device__ inline bool expand_word(CellWord w, uint32_t T, const FfRatio &ff, Metric metric, mr_label_record &o) {
    if (w == kViaSource) {
        o = mr_label_record{0u, 0u, 0u, kViaSource};
        return true;
    }
    if (w & kViaSpecial) {
        const uint32_t t = w & kNone10;
        if (t >= T || (w & ~(kViaSpecial | kNone10))) return false;
        o = mr_label_record{metric(t, 0u), metric(t, 1u), metric(t, 2u), w};
        return true;
    }
    const uint32_t b = w >> kStBShift, k = w & kStKMask;
    if (b >= T) return false;
    const uint32_t run = ff.num == ff.den ? 180u * k : uint32_t((uint64_t(180) * k * ff.num + ff.den - 1) / ff.den);
    o = mr_label_record{metric(b, 0u) + k, metric(b, 1u), metric(b, 2u) + run, b};
    return true;
}

// ---- wire rows (mr_engine.hpp: Wire records) ----
// The header of wire row `row` (max_cmds mc; wp: the wire pool of pool_n commands).  A
// label: nc commands of two words each at src, the first one's `from` rank in `from`.  A
// status row: `status`.  Else the row is malformed: a pool reference past the pool (or with
// no slot to hold it), or an in-slot count above mc.  The commands themselves are not looked
// at (see cmd_cost for who range-checks them).
enum class WireHead { label, status, bad_pool, bad_count };
__host__ __device__ inline WireHead wire_head(const uint32_t *row, uint32_t mc, const uint32_t *wp, uint64_t pool_n,
                                              uint32_t &from, const uint32_t *&src, uint32_t &nc, int32_t &status) {
    const uint32_t code = row[0] >> kWireRankBits;
    from = row[0] & kWireRankMask;
    src = row + 1;
    nc = 0;
    status = MR_OK;
    if (code >= kWireStatus) {
        status = int32_t(code) - int32_t(kWireStatus) - 32;
        return WireHead::status;
    }
    if (code == kWireOvf) {
        if (!mc || uint64_t(row[1]) + row[2] > pool_n) return WireHead::bad_pool;
        src = wp + 2ull * row[1];
        nc = row[2];
    } else {
        if (code > mc) return WireHead::bad_count;
        nc = code;
    }
    return WireHead::label;
}

}  // namespace mr
