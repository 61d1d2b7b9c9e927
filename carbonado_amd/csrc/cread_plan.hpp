// cread_plan.hpp — host logic of include/carbonado_hip_cread.h: the argument
// checks of chipc_ctr_ranges_dev in the order the header fixes, the scratch
// layout and the table a call uploads.  Pure host code (no HIP): it is compiled
// into api_cread.cpp and, stand-alone under ASan + UBSan, into
// tests/cread_device_check.cpp.
//
// Scratch of a call, in this order (every region 16-B aligned):
//   items  [nitems]  cread::Item    public: offsets, positions, lengths, work ranges
//   keys   [nkeys]   RAW_KEY (48) B key (32) || IV (16) of the keys some item uses
//   km     [nkeys]   cread::CtrKey  round keys and J0
// items and keys are one upload.  [keys, total) is the key region: the last
// operation a call enqueues overwrites it with zeros.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "carbonado_hip_cread.h"
#include "cread_device.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace cread {

using rules::ENV_OVERHEAD;  // eph_pub65 || nonce16 || tag16 in front of the ciphertext
using rules::ranges_overlap;
using rules::up16;

constexpr uint64_t MAX_ITEMS = uint64_t(1) << 31;
constexpr uint64_t MAX_WORK = uint64_t(1) << 31;
constexpr uint64_t MAX_OFF = uint64_t(1) << 53;
constexpr uint64_t HDR_LEN = 81;       // eph_pub65 || nonce16
constexpr uint64_t HDR_PITCH = 96;     // a header's slot in the scratch

struct Layout {
    uint64_t items = 0, keys = 0, km = 0, total = 0;
    uint64_t upload_len() const { return km; }
    uint64_t wipe_from() const { return keys; }
    uint64_t wipe_len() const { return total - keys; }
};

inline Layout layout(uint64_t nkeys, uint64_t nitems) {
    Layout l;
    l.items = 0;
    l.keys = up16(nitems * sizeof(Item));
    l.km = l.keys + nkeys * RAW_KEY;
    l.total = l.km + nkeys * sizeof(CtrKey);
    return l;
}

inline uint64_t scratch_len(uint64_t nkeys, uint64_t nitems) {
    if (nitems >= MAX_ITEMS || nkeys > (uint64_t(1) << 32)) return 0;
    return layout(nkeys, nitems).total;
}

struct Plan {
    Layout lay;
    uint64_t nitems = 0, work = 0;
    uint32_t keys_used = 0;
    std::vector<uint8_t> table;  // items || keys: holds key bytes, the caller wipes it
};

// The checks of chipc_ctr_ranges_dev and the call's table.  kill (optional, the
// read): item i with kill[i] != 0 gets zeros and that status, and uses no key.
// Only the keys some item uses go into the table, renumbered in order of first
// use.
inline int plan_ctr(const uint8_t *keys, const uint8_t *ivs, uint64_t nkeys, const uint32_t *item_key,
                    const uint64_t *pos, const uint64_t *n, uint64_t nitems, uintptr_t d_buf, const uint64_t *buf_off,
                    uintptr_t d_scratch, uint64_t scratch_len_given, const uint32_t *kill, Plan *p) {
    if (!keys || !ivs || !item_key || !pos || !n || !buf_off || !d_scratch) return CHIP_ERR_INVALID_ARG;
    if (nitems >= MAX_ITEMS) return CHIP_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nitems; ++i)
        if (item_key[i] >= nkeys) return CHIP_ERR_INVALID_ARG;
    uint64_t work = 0;
    bool any = false;
    for (uint64_t i = 0; i < nitems; ++i) {
        if (pos[i] > MAX_END || n[i] > MAX_END - pos[i]) return CHIP_ERR_INVALID_ARG;
        work += work_of(n[i], kill ? kill[i] : 0);
        if (work >= MAX_WORK) return CHIP_ERR_INVALID_ARG;
        any |= n[i] != 0;
    }
    for (uint64_t i = 0; i < nitems; ++i)
        if (buf_off[i] > MAX_OFF) return CHIP_ERR_INVALID_ARG;
    if (any && !d_buf) return CHIP_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nitems; ++i)
        if (n[i] && ((d_buf + buf_off[i]) & 15u)) return CHIP_ERR_INVALID_ARG;
    if (d_scratch & 15u) return CHIP_ERR_INVALID_ARG;
    if (ranges_overlap(buf_off, n, nitems)) return CHIP_ERR_INVALID_ARG;
    p->lay = layout(nkeys, nitems);
    if (nkeys > (uint64_t(1) << 32) || scratch_len_given < p->lay.total) return CHIP_ERR_INVALID_ARG;
    p->nitems = nitems;
    p->work = work;
    p->table.assign(p->lay.upload_len(), 0);
    std::vector<uint32_t> slot(nkeys, ~uint32_t(0));
    uint32_t used = 0;
    uint64_t w = 0;
    for (uint64_t i = 0; i < nitems; ++i) {
        Item it{};
        it.buf_off = buf_off[i];
        it.pos = pos[i];
        it.n = n[i];
        it.work0 = uint32_t(w);
        it.kill = kill ? kill[i] : 0;
        w += work_of(it.n, it.kill);
        if (it.n && !it.kill) {
            uint32_t &s = slot[item_key[i]];
            if (s == ~uint32_t(0)) {
                s = used++;
                std::memcpy(p->table.data() + p->lay.keys + uint64_t(s) * RAW_KEY, keys + 32ull * item_key[i], 32);
                std::memcpy(p->table.data() + p->lay.keys + uint64_t(s) * RAW_KEY + 32, ivs + 16ull * item_key[i], 16);
            }
            it.key = s;
        }
        std::memcpy(p->table.data() + p->lay.items + i * sizeof(Item), &it, sizeof it);
    }
    p->keys_used = used;
    return CHIP_OK;
}

// ---- the read: plaintext requests as envelope requests ------------------------------
// start[r] + 97 of every request (plaintext byte x is envelope byte x + 97; the
// ranged read clips at the envelope's end, which is the plaintext's); a start
// that would wrap becomes the largest value, which the ranged read refuses
inline std::vector<uint64_t> shifted(const uint64_t *start, uint64_t nreq) {
    const uint64_t top = ~uint64_t(0);
    std::vector<uint64_t> s(nreq);
    for (uint64_t r = 0; r < nreq; ++r) s[r] = start[r] > top - ENV_OVERHEAD ? top : start[r] + ENV_OVERHEAD;
    return s;
}

}  // namespace cread
}  // namespace chip
