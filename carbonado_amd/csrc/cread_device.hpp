// cread_device.hpp — AES-256-GCM's keystream at any byte offset, XORed over
// ranges in place: the arithmetic of KC (cread_kernels.hip).  Everything here
// is built from gcm_device.hpp as it stands (the bitsliced AES, gf128_mul,
// counter_block, load_block / store_block) and keeps its rule: no load or store
// address and no branch depends on a key, a round key, H, J0 or keystream.
// Positions, lengths, offsets, gate and kill words are public and do.
//
// Every function is __host__ __device__: the kernels and the stand-alone check
// tests/cread_device_check.cpp compile this same text, the check walking an
// item lane by lane exactly as the kernels split it, the neighbour exchange
// included.
//
// How an item is split.  Item i XORs n bytes at a 16-B aligned address with
// keystream bytes [pos, pos + n) of its key.  Its UNIT u is the 16 buffer bytes
// [16 u, 16 u + 16) (the last one may be short); with b0 = pos / 16 and
// sh = pos % 16 unit u needs keystream blocks b0 + u and, when sh != 0,
// b0 + u + 1: bytes sh .. 15 of the first, 0 .. sh - 1 of the second.  A WORK
// ITEM is (item, span): units [127 span, 127 span + 127) on one wave.  Lane l
// evaluates the disjoint pair of blocks (2 l, 2 l + 1) of the span in one
// bitsliced evaluation (lane_eval), takes block 2 l + 2 from lane l + 1 (a
// lane shuffle on the device, an array index in the check) and serves units
// 2 l and 2 l + 1 (lane_apply); lane 63 has no neighbour and serves unit 126
// alone.  So a wave's 64 evaluations give 128 blocks and serve 127 units, where
// evaluating each unit's own pair would serve 64.
#pragma once

#include "gcm_device.hpp"

namespace chip {
namespace cread {

constexpr uint32_t LANES = gcm::LANES;
constexpr uint32_t SPAN_UNITS = 2 * LANES - 1;  // units of a work item
constexpr uint64_t MAX_END = (uint64_t(1) << 36) - 32;  // GCM's limit on one message
constexpr uint64_t RAW_KEY = 48;  // a raw key record: key (32) || IV (16), as ctr_setup_kernel reads it

// What a read needs of a key: no power of H (a read hashes nothing with it).
struct CtrKey {
    uint32_t rk[gcm::RK_WORDS];  // bitsliced round keys, both block positions alike
    uint32_t j0[4];              // J0 as four little-endian words of its bytes
    uint32_t pad_[4];
};
static_assert(sizeof(CtrKey) == 512, "record layout");

// One item of a call (public: offsets, positions and lengths only).
struct Item {
    uint64_t buf_off;  // of its first byte in the call's buffer; the address is 16-B aligned
    uint64_t pos;      // of that byte in its key's message
    uint64_t n;
    uint32_t work0;    // its work items are [work0, work0 + work_of(n, kill)) of the call
    uint32_t key;      // index into the call's (compacted) keys; unused by a killed item
    uint32_t kill;     // decided on the host (the read): != 0: zeros over the range, this status, no keystream
    uint32_t pad_;
};
static_assert(sizeof(Item) == 40, "record layout");

GCM_HD uint64_t units_of(uint64_t n) { return (n + 15) / 16; }
GCM_HD uint64_t spans_of(uint64_t n) { return (units_of(n) + SPAN_UNITS - 1) / SPAN_UNITS; }
// a killed item has a work item even when it is empty: its status words are written by one
GCM_HD uint64_t work_of(uint64_t n, uint32_t kill) {
    const uint64_t s = spans_of(n);
    return kill && !s ? 1 : s;
}

// ---- key setup, without the powers ---------------------------------------------
// rk: the expanded key (aes256_expand).  J0 = GHASH_H(IV || 0^64 || [128]_64):
// H = E_K(0) and two multiplications.
GCM_HD void setup_lite(const uint32_t *rk, const uint8_t iv[16], uint32_t j0[4]) {
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    gcm::aes256_encrypt2(rk, q);
    const uint32_t hle[4] = {q[0], q[2], q[4], q[6]};
    const gcm::B128 H = gcm::gf128_from_le(hle);
    uint32_t ivle[4];
    GCM_UNROLL
    for (int c = 0; c < 4; ++c)
        ivle[c] = uint32_t(iv[4 * c]) | uint32_t(iv[4 * c + 1]) << 8 | uint32_t(iv[4 * c + 2]) << 16 |
                  uint32_t(iv[4 * c + 3]) << 24;
    gcm::B128 y = gcm::gf128_mul(gcm::gf128_from_le(ivle), H);
    y.w[3] ^= 128u;
    y = gcm::gf128_mul(y, H);
    GCM_UNROLL
    for (int c = 0; c < 4; ++c) j0[c] = gcm::bswap32(y.w[c]);
}

// ---- keystream bytes at a byte offset --------------------------------------------
// bytes [sh, sh + 16) of a || b (blocks as four little-endian words), sh < 16.
// The words move down by sh / 4 places under masks, one stage per bit of that
// count (an index into the words would put the keystream into memory at an
// address computed at run time), then by 8 (sh % 4) bits.
GCM_HD void ks_shift(const uint32_t a[4], const uint32_t b[4], uint32_t sh, uint32_t out[4]) {
    const uint32_t ws = sh >> 2, bs = 8 * (sh & 3u);
    const uint32_t m1 = 0u - (ws & 1u), m2 = 0u - ((ws >> 1) & 1u);
    uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    GCM_UNROLL
    for (uint32_t j = 0; j < 7; ++j) w[j] = (w[j] & ~m1) | (w[j + 1] & m1);
    GCM_UNROLL
    for (uint32_t j = 0; j < 5; ++j) w[j] = (w[j] & ~m2) | (w[j + 2] & m2);
    GCM_UNROLL
    for (uint32_t j = 0; j < 4; ++j) out[j] = (w[j] >> bs) | ((w[j + 1] << 1) << (31 - bs));
}

// ---- one lane of one work item ------------------------------------------------------
// units of the item in this span
GCM_HD uint32_t span_units(const Item &it, uint32_t span) {
    const uint64_t left = units_of(it.n) - uint64_t(span) * SPAN_UNITS;
    return uint32_t(left < SPAN_UNITS ? left : SPAN_UNITS);
}
// whether some unit of the span needs one of the lane's two blocks
GCM_HD bool lane_needed(const Item &it, uint32_t span, uint32_t lane) {
    return 2 * lane < span_units(it, span) + ((it.pos & 15u) ? 1u : 0u);
}
// blocks 2 lane and 2 lane + 1 of the span: E_K of their counter blocks
GCM_HD void lane_eval(const CtrKey *k, const Item &it, uint32_t span, uint32_t lane, uint32_t ka[4], uint32_t kb[4]) {
    const uint64_t b = it.pos / 16 + uint64_t(span) * SPAN_UNITS + 2 * lane;
    uint32_t ca[4], cb[4];
    gcm::counter_block(k->j0, b, ca);
    gcm::counter_block(k->j0, b + 1, cb);
    uint32_t q[8] = {ca[0], cb[0], ca[1], cb[1], ca[2], cb[2], ca[3], cb[3]};
    gcm::aes256_encrypt2(k->rk, q);
    GCM_UNROLL
    for (int c = 0; c < 4; ++c) {
        ka[c] = q[2 * c];
        kb[c] = q[2 * c + 1];
    }
}
// unit u of the item (it exists): buf ^= bytes [sh, sh + 16) of first || second
GCM_HD void unit_apply(const Item &it, uint64_t u, const uint32_t first[4], const uint32_t second[4], uint8_t *buf) {
    const uint64_t left = it.n - 16 * u;
    const uint32_t nb = uint32_t(left < 16 ? left : 16);
    uint32_t ks[4], c[4];
    ks_shift(first, second, uint32_t(it.pos & 15u), ks);
    gcm::load_block(buf + 16 * u, nb, c);
    GCM_UNROLL
    for (int j = 0; j < 4; ++j) c[j] ^= ks[j];
    gcm::store_block(buf + 16 * u, c, nb);
}
// ka, kb: the lane's own blocks; kn: block 2 lane + 2, lane + 1's first (not
// looked at by lane 63, nor where pos % 16 == 0).  buf: the item's first byte.
GCM_HD void lane_apply(const Item &it, uint32_t span, uint32_t lane, const uint32_t ka[4], const uint32_t kb[4],
                       const uint32_t kn[4], uint8_t *buf) {
    const uint32_t nu = span_units(it, span);
    const uint64_t u0 = uint64_t(span) * SPAN_UNITS;
    if (2 * lane < nu) unit_apply(it, u0 + 2 * lane, ka, kb, buf);
    if (lane + 1 < LANES && 2 * lane + 1 < nu) unit_apply(it, u0 + 2 * lane + 1, kb, kn, buf);
}
// a killed item: zeros over the lane's units
GCM_HD void lane_zero(const Item &it, uint32_t span, uint32_t lane, uint8_t *buf) {
    if (!it.n) return;
    const uint32_t nu = span_units(it, span);
    const uint64_t u0 = uint64_t(span) * SPAN_UNITS;
    const uint32_t z[4] = {0, 0, 0, 0};
    GCM_UNROLL
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t x = 2 * lane + j;
        if (x >= nu || x >= SPAN_UNITS) continue;
        const uint64_t left = it.n - 16 * (u0 + x);
        gcm::store_block(buf + 16 * (u0 + x), z, uint32_t(left < 16 ? left : 16));
    }
}
// a killed item on one lane: no keystream, zeros over the lane's units, and by
// span 0 the item's result words, i its index in them.  KC's wave finds the
// item in its table, KK's builds it from the request; both end here.  Plain
// stores and no lane exchange, so it stands with the other lane functions and
// the host check runs it.
GCM_HD void lane_kill(const Item &it, uint32_t span, uint32_t lane, uint8_t *buf, uint32_t *status, uint32_t *used,
                      uint32_t *vouch, uint32_t i) {
    if (span == 0 && lane == 0) {
        status[i] = it.kill;
        used[i] = 0;
        vouch[i] = 0;
    }
    lane_zero(it, span, lane, buf);
}

// the item of work item w: the last one whose work0 is not behind it (items
// without work share a neighbour's work0 and are never found)
GCM_HD uint32_t item_of(const Item *items, uint32_t nitems, uint32_t w) {
    uint32_t lo = 0, hi = nitems - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (items[mid].work0 <= w) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace cread
}  // namespace chip
