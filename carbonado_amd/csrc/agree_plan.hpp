// agree_plan.hpp — host logic of include/carbonado_hip_agree.h: the argument
// checks of the two raw key calls in the order the header fixes, the scratch
// layout, the scalar checks and the tables a call uploads.  Pure host code (no
// HIP): it is compiled into api_agree.cpp and, stand-alone under ASan + UBSan,
// into tests/agree_device_check.cpp.
//
// Agreement scratch of a call over `count` objects, in this order (every
// region 16-B aligned):
//   ptab   96 KiB                 public: the comb table of the receiver's key (seal)
//   vtab   [ceil64(count)] 1536 B public: 16 multiples of every ephemeral key (open)
//   sk     [count] 32 B           the scalars, eight little-endian words each
//                                 (open: the receiver's alone, in slot 0)
// [sk, total) is the key region: the last operation a call enqueues overwrites
// it with zeros.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "agree_device.hpp"
#include "carbonado_hip.h"
#include "secp256k1_host.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace agree {

constexpr uint64_t MAX_COUNT = uint64_t(1) << 31;
constexpr uint64_t MAX_PITCH = uint64_t(1) << 32;

struct KeysLayout {
    uint64_t ptab = 0, vtab = 0, sk = 0, total = 0;
    uint64_t wipe_from() const { return sk; }
    uint64_t wipe_len() const { return total - sk; }
};

inline KeysLayout keys_layout(uint64_t count) {
    KeysLayout l;
    l.ptab = 0;
    l.vtab = uint64_t(COMB_WORDS) * 4;
    l.sk = l.vtab + var_words(count) * 4;
    l.total = l.sk + 32 * count;
    return l;
}

inline uint64_t keys_scratch_len(uint64_t count) {
    if (count == 0 || count >= MAX_COUNT) return 0;
    return keys_layout(count).total;
}

// 0 < k < n for 32 big-endian bytes (SecretKey::parse); one pass, no early exit
inline bool scalar_ok(const uint8_t k[32]) {
    static const uint8_t N_BE[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,
                                     0xFF, 0xFF, 0xFF, 0xFF, 0xFE, 0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48,
                                     0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41};
    int borrow = 0;
    unsigned any = 0;
    for (int i = 31; i >= 0; --i) {  // k - n: a borrow out means k < n
        const int d = int(k[i]) - int(N_BE[i]) - borrow;
        borrow = d < 0;
        any |= k[i];
    }
    return borrow && any;
}

// 32 big-endian bytes -> the eight little-endian words the kernels read
inline void scalar_words(const uint8_t k[32], uint8_t out[32]) {
    for (int i = 0; i < 8; ++i) {
        const uint8_t *q = k + 4 * (7 - i);
        const uint32_t w = (uint32_t(q[0]) << 24) | (uint32_t(q[1]) << 16) | (uint32_t(q[2]) << 8) | q[3];
        std::memcpy(out + 4 * i, &w, 4);
    }
}

inline void fe_words(const k1::Fe &f, uint32_t out[8]) {
    uint8_t be[32];
    k1::fe_to_be(f, be);
    const Fe v = fe_from_be(be);
    std::memcpy(out, v.v, 32);
}

// a host comb table (i 16^j B, projective, five 52-bit limbs) as the COMB_WORDS words comb_pick reads
inline void fill_comb(const k1::CombTable &t, uint32_t *out) {
    for (int j = 0; j < 64; ++j)
        for (int i = 0; i < 16; ++i) {
            uint32_t *e = out + (size_t(j) * 16 + i) * PT_WORDS;
            fe_words(t.t[j][i].x, e);
            fe_words(t.t[j][i].y, e + 8);
            fe_words(t.t[j][i].z, e + 16);
        }
}

// The checks of chipy_seal_keys_dev that need no key, in the header's order.
inline int check_seal_keys(bool have, uint64_t count, uint64_t pub_pitch, uint64_t key_pitch, uintptr_t d_scratch,
                           uint64_t scratch_len) {
    if (!have || count >= MAX_COUNT) return CHIP_ERR_INVALID_ARG;
    if (pub_pitch < 65 || pub_pitch > MAX_PITCH || key_pitch < 32 || key_pitch > MAX_PITCH) return CHIP_ERR_INVALID_ARG;
    if (d_scratch & 15u) return CHIP_ERR_INVALID_ARG;
    if (scratch_len < keys_layout(count).total) return CHIP_ERR_INVALID_ARG;
    return CHIP_OK;
}

// ... of chipy_open_keys_dev (the pitches: the ephemeral keys', the keys')
inline int check_open_keys(bool have, uint64_t count, uint64_t eph_pitch, uint64_t key_pitch, uintptr_t d_scratch,
                           uint64_t scratch_len) {
    return check_seal_keys(have, count, eph_pitch, key_pitch, d_scratch, scratch_len);
}

}  // namespace agree
}  // namespace chip
