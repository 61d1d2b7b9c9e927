// snap_plan.hpp — host side of the snappy calls of
// include/carbonado_hip_snap.h: the argument checks in the header's order, the
// scratch layouts and the tables the kernels of snap_kernels.hip read.  Pure
// host code (no HIP): addresses are plain integers here, so the host check
// (tests/snap_device_check.cpp) runs it without a device.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/carbonado_hip.h"
#include "snap_device.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace snap {

using rules::ranges_overlap;
using rules::up16;

constexpr uint64_t MAX_COUNT = uint64_t(1) << 31;
constexpr uint64_t MAX_LEN = uint64_t(1) << 40;     // an object, a stream or a capacity
constexpr uint64_t MAX_OFFSET = uint64_t(1) << 53;
constexpr uint64_t MAX_ITEMS = uint64_t(1) << 31;   // blocks (compress) or slots (decompress) of a call
constexpr uint64_t STREAM_ID_LEN = 10;

inline uint64_t blocks_of(uint64_t n) { return (n + MAX_BLOCK - 1) / MAX_BLOCK; }
// chip_snap_max_len
inline uint64_t max_len(uint64_t n) { return n == 0 ? 0 : STREAM_ID_LEN + 8 * blocks_of(n) + n; }
// data chunks a stream may have: every stream FrameEncoder or this library writes fits
inline uint64_t slots_of(uint64_t out_cap) { return blocks_of(out_cap) + 1; }

// ---- compress: [objs | blks] uploaded, then [meta | slots]
struct CLayout {
    uint64_t objs = 0, blks = 0, meta = 0, slots = 0, total = 0;
    CLayout() = default;
    CLayout(uint64_t count, uint64_t blocks) {
        blks = up16(count * sizeof(CObj));
        meta = blks + up16(blocks * sizeof(CBlk));
        slots = meta + up16(blocks * sizeof(CMeta));
        total = slots + blocks * SLOT_PITCH;
    }
    uint64_t table_len() const { return meta; }
};

struct CPlan {
    std::vector<uint8_t> table;
    uint64_t count = 0, blocks = 0;
    CLayout lay;
};

// false for lengths no call accepts
inline bool count_blocks(const uint64_t *n, uint64_t count, uint64_t *blocks) {
    if (!n || count == 0 || count >= MAX_COUNT) return false;
    uint64_t b = 0;
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > MAX_LEN) return false;
        b += blocks_of(n[o]);
        if (b >= MAX_ITEMS) return false;
    }
    *blocks = b;
    return true;
}

inline uint64_t snap_scratch_len(const uint64_t *n, uint64_t count) {
    uint64_t b;
    return count_blocks(n, count, &b) ? CLayout(count, b).total : 0;
}

// chips_snap_ragged_dev's checks (count > 0) and table
inline int plan_snap(uintptr_t d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count, uintptr_t d_out,
                     const uint64_t *out_off, bool have_out_len, uintptr_t d_scratch, uint64_t scratch_len, CPlan *p) {
    if (!in_off || !n || !out_off || !have_out_len || !d_scratch || count >= MAX_COUNT) return CHIP_ERR_INVALID_ARG;
    uint64_t blocks;
    if (!count_blocks(n, count, &blocks)) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> worst(count);
    for (uint64_t o = 0; o < count; ++o) {
        worst[o] = max_len(n[o]);
        if (n[o] && (!d_in || !d_out)) return CHIP_ERR_INVALID_ARG;
    }
    for (uint64_t o = 0; o < count; ++o)
        if (in_off[o] > MAX_OFFSET || out_off[o] > MAX_OFFSET) return CHIP_ERR_INVALID_ARG;
    for (uint64_t o = 0; o < count; ++o)
        if (n[o] && ((d_in + in_off[o]) & 15)) return CHIP_ERR_INVALID_ARG;
    if (d_scratch & 15) return CHIP_ERR_INVALID_ARG;
    if (ranges_overlap(out_off, worst.data(), count)) return CHIP_ERR_INVALID_ARG;
    p->count = count;
    p->blocks = blocks;
    p->lay = CLayout(count, blocks);
    if (scratch_len < p->lay.total) return CHIP_ERR_INVALID_ARG;
    p->table.assign(p->lay.table_len(), 0);
    CObj *objs = reinterpret_cast<CObj *>(p->table.data() + p->lay.objs);
    CBlk *blks = reinterpret_cast<CBlk *>(p->table.data() + p->lay.blks);
    uint64_t b = 0;
    for (uint64_t o = 0; o < count; ++o) {
        const uint64_t nb = blocks_of(n[o]);
        objs[o].in_off = in_off[o];
        objs[o].n = n[o];
        objs[o].out_off = out_off[o];
        objs[o].blk0 = uint32_t(b);
        objs[o].nblk = uint32_t(nb);
        for (uint64_t k = 0; k < nb; ++k) {
            blks[b + k].obj = uint32_t(o);
            blks[b + k].idx = uint32_t(k);
        }
        b += nb;
    }
    return CHIP_OK;
}

// ---- decompress: [objs | slot_obj] uploaded, then [desc | bad | state]
struct ULayout {
    uint64_t objs = 0, slot_obj = 0, desc = 0, bad = 0, state = 0, total = 0;
    ULayout() = default;
    ULayout(uint64_t count, uint64_t slots) {
        slot_obj = up16(count * sizeof(UObj));
        desc = slot_obj + up16(slots * sizeof(uint32_t));
        bad = desc + up16(slots * sizeof(UDesc));
        state = bad + up16(slots * sizeof(uint32_t));
        total = state + up16(count * sizeof(UState));
    }
    uint64_t table_len() const { return desc; }
};

struct UPlan {
    std::vector<uint8_t> table;
    uint64_t count = 0, slots = 0;
    ULayout lay;
};

inline bool count_slots(const uint64_t *in_len, const uint64_t *out_cap, uint64_t count, uint64_t *slots) {
    if (!in_len || !out_cap || count == 0 || count >= MAX_COUNT) return false;
    uint64_t s = 0;
    for (uint64_t o = 0; o < count; ++o) {
        if (in_len[o] > MAX_LEN || out_cap[o] > MAX_LEN) return false;
        s += slots_of(out_cap[o]);
        if (s >= MAX_ITEMS) return false;
    }
    *slots = s;
    return true;
}

inline uint64_t unsnap_scratch_len(const uint64_t *in_len, const uint64_t *out_cap, uint64_t count) {
    uint64_t s;
    return count_slots(in_len, out_cap, count, &s) ? ULayout(count, s).total : 0;
}

// chips_unsnap_ragged_dev's checks (count > 0) and table
inline int plan_unsnap(uintptr_t d_in, const uint64_t *in_off, const uint64_t *in_len, uint64_t count, uintptr_t d_out,
                       const uint64_t *out_off, const uint64_t *out_cap, bool have_out_len, bool have_status,
                       uintptr_t d_scratch, uint64_t scratch_len, UPlan *p) {
    if (!in_off || !in_len || !out_off || !out_cap || !have_out_len || !have_status || !d_scratch ||
        count >= MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    uint64_t slots;
    if (!count_slots(in_len, out_cap, count, &slots)) return CHIP_ERR_INVALID_ARG;
    for (uint64_t o = 0; o < count; ++o)
        if ((in_len[o] && !d_in) || (out_cap[o] && !d_out)) return CHIP_ERR_INVALID_ARG;
    for (uint64_t o = 0; o < count; ++o)
        if (in_off[o] > MAX_OFFSET || out_off[o] > MAX_OFFSET) return CHIP_ERR_INVALID_ARG;
    for (uint64_t o = 0; o < count; ++o)
        if (out_cap[o] && ((d_out + out_off[o]) & 15)) return CHIP_ERR_INVALID_ARG;
    if (d_scratch & 15) return CHIP_ERR_INVALID_ARG;
    if (ranges_overlap(out_off, out_cap, count)) return CHIP_ERR_INVALID_ARG;
    p->count = count;
    p->slots = slots;
    p->lay = ULayout(count, slots);
    if (scratch_len < p->lay.total) return CHIP_ERR_INVALID_ARG;
    p->table.assign(p->lay.table_len(), 0);
    UObj *objs = reinterpret_cast<UObj *>(p->table.data() + p->lay.objs);
    uint32_t *slot_obj = reinterpret_cast<uint32_t *>(p->table.data() + p->lay.slot_obj);
    uint64_t s = 0;
    for (uint64_t o = 0; o < count; ++o) {
        const uint64_t ns = slots_of(out_cap[o]);
        objs[o].in_off = in_off[o];
        objs[o].in_len = in_len[o];
        objs[o].out_off = out_off[o];
        objs[o].out_cap = out_cap[o];
        objs[o].slot0 = uint32_t(s);
        objs[o].nslots = uint32_t(ns);
        for (uint64_t k = 0; k < ns; ++k) slot_obj[s + k] = uint32_t(o);
        s += ns;
    }
    return CHIP_OK;
}

// ---- the one-call forms (formats 6, 7, 10, 11, 14, 15)
inline bool snap_format(uint8_t f) {
    return f < 16 && (f & CHIP_FORMAT_SNAPPY) && (f & (CHIP_FORMAT_BAO | CHIP_FORMAT_ZFEC));
}
using rules::ENV_OVERHEAD;                             // the Ecies envelope around a frame stream
constexpr uint64_t MAX_STAGE = uint64_t(16) << 20;     // what enters zfec / bao, per object

// what enters zfec / bao at worst for an n-byte object
inline uint64_t worst_stage_len(uint8_t format, uint64_t n) {
    return max_len(n) + ((format & CHIP_FORMAT_ECIES) ? ENV_OVERHEAD : 0);
}

}  // namespace snap
}  // namespace chip
