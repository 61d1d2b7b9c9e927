// ecies_plan.hpp — host logic of include/carbonado_hip_ecies.h: the argument
// checks of the raw AES-256-GCM calls in the order the header fixes, the
// scratch layout and the table a call uploads.  Pure host code (no HIP): it is
// compiled into api_ecies.cpp and, stand-alone under ASan + UBSan, into
// tests/gcm_device_check.cpp.
//
// Scratch of a call, in this order (every region 16-B aligned):
//   msgs   [count]  gcm::Msg      public: offsets, lengths, item ranges
//   hdrs   [count]  96 B          public: the 81 header bytes of an envelope
//   keys   [count]  48 B          key (32) || IV (16) as the caller gave them
//   km     [count]  gcm::KeyMat   round keys, powers of H, J0, E_K(J0)
//   vals   [items]  16 B          GHASH values of the items
//   ok     [count]  u32           verdict words (open)
// msgs, hdrs and keys are one upload.  [keys, ok) is the key region: the last
// operation a call enqueues overwrites it with zeros.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "carbonado_hip_ecies.h"
#include "gcm_device.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace ecies {

using rules::ranges_overlap;
using rules::up16;

constexpr uint64_t MAX_COUNT = uint64_t(1) << 31;
constexpr uint64_t MAX_MSG = (uint64_t(1) << 36) - 32;  // GCM's limit on one message
constexpr uint64_t MAX_ITEMS = uint64_t(1) << 31;
constexpr uint64_t HDR_LEN = 81;    // eph_pub65 || nonce16 of an envelope
constexpr uint64_t HDR_PITCH = 96;  // its slot in the scratch
using rules::ENV_OVERHEAD;          // ... || tag16

struct Layout {
    uint64_t msgs = 0, hdrs = 0, keys = 0, km = 0, vals = 0, ok = 0, total = 0;
    uint64_t upload_len() const { return km; }
    uint64_t wipe_from() const { return keys; }
    uint64_t wipe_len() const { return ok - keys; }
};

inline Layout layout(uint64_t count, uint64_t items) {
    Layout l;
    l.msgs = 0;
    l.hdrs = up16(count * sizeof(gcm::Msg));
    l.keys = l.hdrs + count * HDR_PITCH;
    l.km = l.keys + count * 48;
    l.vals = l.km + count * sizeof(gcm::KeyMat);
    l.ok = l.vals + items * 16;
    l.total = l.ok + up16(count * 4);
    return l;
}

// items of a set of lengths; false when a length or the sum is out of range
inline bool count_items(const uint64_t *len, uint64_t count, uint64_t *items) {
    uint64_t t = 0;
    for (uint64_t o = 0; o < count; ++o) {
        if (len[o] > MAX_MSG) return false;
        t += gcm::items_of(len[o]);
        if (t >= MAX_ITEMS) return false;
    }
    *items = t;
    return true;
}

inline uint64_t gcm_scratch_len(const uint64_t *len, uint64_t count) {
    uint64_t items = 0;
    if (count == 0 || !len || count >= MAX_COUNT || !count_items(len, count, &items)) return 0;
    return layout(count, items).total;
}

struct Plan {
    Layout lay;
    uint64_t count = 0, items = 0;
    std::vector<uint8_t> table;  // msgs || hdrs || keys: holds key bytes, the caller wipes it
};

// The checks of chipe_gcm_seal_ragged_dev (seal) / chipe_gcm_open_ragged_dev
// and the call's table.  d_plain is the side that wants 16-B alignment: the
// input of a seal, the output of an open.  tag_off: NULL for tags at 16 o.
// refused (optional): messages that fail whatever their tag.
inline int plan_gcm(bool seal, const uint8_t *keys, const uint8_t *ivs, uintptr_t d_in, const uint64_t *in_off,
                    const uint64_t *len, uint64_t count, uintptr_t d_out, const uint64_t *out_off, uintptr_t d_tag,
                    const uint64_t *tag_off, bool status_ok, uintptr_t d_scratch, uint64_t scratch_len, Plan *p,
                    const uint8_t *refused = nullptr) {
    if (!keys || !ivs || !in_off || !len || !out_off || !d_tag || !status_ok || !d_scratch) return CHIP_ERR_INVALID_ARG;
    if (count >= MAX_COUNT) return CHIP_ERR_INVALID_ARG;
    uint64_t items = 0;
    if (!count_items(len, count, &items)) return CHIP_ERR_INVALID_ARG;
    bool any = false;
    for (uint64_t o = 0; o < count; ++o) any |= len[o] != 0;
    if (any && (!d_in || !d_out)) return CHIP_ERR_INVALID_ARG;
    const uintptr_t d_plain = seal ? d_in : d_out;
    const uint64_t *plain_off = seal ? in_off : out_off;
    for (uint64_t o = 0; o < count; ++o) {
        if (in_off[o] > (uint64_t(1) << 53) || out_off[o] > (uint64_t(1) << 53)) return CHIP_ERR_INVALID_ARG;
        if (len[o] && ((d_plain + plain_off[o]) & 15u)) return CHIP_ERR_INVALID_ARG;
    }
    if (d_scratch & 15u) return CHIP_ERR_INVALID_ARG;
    if (ranges_overlap(out_off, len, count)) return CHIP_ERR_INVALID_ARG;
    p->lay = layout(count, items);
    if (scratch_len < p->lay.total) return CHIP_ERR_INVALID_ARG;
    p->count = count;
    p->items = items;
    p->table.assign(p->lay.upload_len(), 0);
    uint64_t item0 = 0;
    for (uint64_t o = 0; o < count; ++o) {
        gcm::Msg m{};
        m.in_off = in_off[o];
        m.out_off = out_off[o];
        m.tag_off = tag_off ? tag_off[o] : 16 * o;
        m.len = len[o];
        m.item0 = uint32_t(item0);
        m.nitems = uint32_t(gcm::items_of(len[o]));
        m.refused = refused && refused[o];
        item0 += m.nitems;
        std::memcpy(p->table.data() + p->lay.msgs + o * sizeof(gcm::Msg), &m, sizeof m);
        std::memcpy(p->table.data() + p->lay.keys + o * 48, keys + 32 * o, 32);
        std::memcpy(p->table.data() + p->lay.keys + o * 48 + 32, ivs + 16 * o, 16);
    }
    return CHIP_OK;
}

// the slots of message o in a plan's table
inline void fill_key(Plan &p, uint64_t o, const uint8_t key[32], const uint8_t iv[16]) {
    std::memcpy(p.table.data() + p.lay.keys + o * 48, key, 32);
    std::memcpy(p.table.data() + p.lay.keys + o * 48 + 32, iv, 16);
}
inline void fill_hdr(Plan &p, uint64_t o, const uint8_t eph_pub[65], const uint8_t iv[16]) {
    std::memcpy(p.table.data() + p.lay.hdrs + o * HDR_PITCH, eph_pub, 65);
    std::memcpy(p.table.data() + p.lay.hdrs + o * HDR_PITCH + 65, iv, 16);
}
inline void set_refused(Plan &p, uint64_t o) {
    const uint32_t one = 1;
    std::memcpy(p.table.data() + p.lay.msgs + o * sizeof(gcm::Msg) + offsetof(gcm::Msg, refused), &one, 4);
}

}  // namespace ecies
}  // namespace chip
