// gcm_device.hpp — AES-256-GCM as ecies 0.2.6 uses it (16-byte nonce, no AAD),
// written so that no load or store address and no branch depends on a secret:
// the key, the round keys, H and its powers, the GHASH accumulator, the
// keystream and the plaintext only ever travel through registers and through
// memory at addresses fixed by the message's index and length.  Ciphertext,
// lengths, offsets and verdict words may drive addresses and branches.
//
// Every function here is __host__ __device__: the kernels of
// ecies_kernels.hip and the stand-alone check tests/gcm_device_check.cpp
// compile this same text, the check walking a message lane by lane exactly as
// the kernels split it.
//
// AES.  No table anywhere.  The state of TWO blocks is held bitsliced in eight
// 32-bit words: word b holds bit b of each of the 32 state bytes, the bit of
// byte (row, col) of block blk at position 8 row + 2 col + blk.  ShiftRows is
// then a rotation inside each byte of a word, MixColumns rotations of whole
// words, and SubBytes a boolean circuit over the eight words: the inverse as
// x^254 (4 bitsliced GF(2^8) multiplications and 7 squarings, polynomial
// basis, x^8 + x^4 + x^3 + x + 1) followed by the affine map.  The circuit is
// checked against the FIPS-197 table for all 256 inputs in all 32 positions.
//
// GHASH.  No Shoup table.  gf128_mul is bit-serial: 128 steps of "add V under
// a mask made from one bit of a, multiply V by x", both branch-free.
// Parallelism comes from powers of H (see the span layout below).
//
// How a message is split.  Its nb = ceil(len / 16) blocks are right-aligned
// in items of SPAN = 64 * RUN blocks (8 KiB): item s covers the virtual blocks
// [s SPAN, (s + 1) SPAN), virtual block v being real block v - Z with
// Z = nitems SPAN - nb, so that only the FIRST item is partial.  Leading
// absent blocks leave a Horner state at zero, so every power below is fixed:
//   lane l of the item's wave absorbs virtual blocks s SPAN + 64 t + l,
//   t = 0 .. RUN - 1, by Horner with H^64, then multiplies by H^(64 - l);
//   the XOR over the 64 lanes is the item's value V_s = sum_j X_j H^(SPAN - j);
//   the message's state is sum_s V_s G^(nitems - 1 - s) with G = H^SPAN,
//   computed the same way by one wave: lane l runs Horner with G^64 over the
//   items 64 t + l of the right-aligned item list and multiplies by
//   G^(63 - l);
//   tag = E_K(J0) ^ (state ^ [0]_64 [8 len]_64) H.
// CTR runs in the same lanes: real block i uses inc32^(i + 1)(J0), two
// blocks (t, t + 1) per bitsliced evaluation.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GCM_HD __host__ __device__ inline
#define GCM_UNROLL _Pragma("unroll")
#define GCM_UNROLL4 _Pragma("unroll 4")
#define GCM_ROLLED _Pragma("unroll 1")
#else
#define GCM_HD inline
#define GCM_UNROLL
#define GCM_UNROLL4
#define GCM_ROLLED
#endif

namespace chip {
namespace gcm {

constexpr uint32_t LANES = 64;          // lanes of a wave
constexpr uint32_t RUN = 8;             // Horner steps of a lane in one item
constexpr uint32_t SPAN = LANES * RUN;  // blocks of an item (8 KiB)
constexpr uint32_t RK_WORDS = 15 * 8;   // bitsliced round keys
constexpr uint32_t MODE_SEAL = 0, MODE_HASH = 1, MODE_CTR = 2;

// An element of GF(2^128) in GCM's order: w[0] bit 31 is the coefficient of
// x^0 (the first bit of the block), w[3] bit 0 that of x^127.
struct B128 {
    uint32_t w[4];
};

// The key material of one message, in the call's scratch (wiped at the end).
struct KeyMat {
    uint32_t rk[RK_WORDS];  // bitsliced round keys, both block positions alike
    B128 hp[LANES + 1];     // H^j
    B128 gp[LANES + 1];     // G^j, G = H^SPAN
    uint32_t j0[4];         // J0 as four little-endian words of its bytes
    uint32_t ej0[4];        // E_K(J0), likewise
};

// One message of a call (public: offsets and lengths only).
struct Msg {
    uint64_t in_off, out_off, tag_off, len;
    uint32_t item0, nitems;  // its items are [item0, item0 + nitems) of the call
    uint32_t refused, pad_;  // refused: decided on the host (open): fails whatever its tag
};

GCM_HD uint32_t bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
GCM_HD uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// ---- GF(2^128) ---------------------------------------------------------------
GCM_HD B128 gf128_mul(const B128 &a, const B128 &b) {
    uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
    uint32_t v0 = b.w[0], v1 = b.w[1], v2 = b.w[2], v3 = b.w[3];
    GCM_UNROLL
    for (int j = 0; j < 4; ++j) {
        uint32_t x = a.w[j];
        GCM_UNROLL4
        for (int i = 0; i < 32; ++i) {
            const uint32_t m = 0u - (x >> 31);
            x <<= 1;
            z0 ^= v0 & m;
            z1 ^= v1 & m;
            z2 ^= v2 & m;
            z3 ^= v3 & m;
            const uint32_t r = 0u - (v3 & 1u);
            v3 = (v3 >> 1) | (v2 << 31);
            v2 = (v2 >> 1) | (v1 << 31);
            v1 = (v1 >> 1) | (v0 << 31);
            v0 = (v0 >> 1) ^ (r & 0xE1000000u);
        }
    }
    return B128{{z0, z1, z2, z3}};
}
GCM_HD B128 gf128_xor(const B128 &a, const B128 &b) {
    return B128{{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}};
}
GCM_HD B128 gf128_one() { return B128{{0x80000000u, 0, 0, 0}}; }
// a block given as four little-endian words of its bytes
GCM_HD B128 gf128_from_le(const uint32_t c[4]) {
    return B128{{bswap32(c[0]), bswap32(c[1]), bswap32(c[2]), bswap32(c[3])}};
}

// ---- bitsliced AES -----------------------------------------------------------
GCM_HD void swapn(uint32_t cl, uint32_t ch, int s, uint32_t &x, uint32_t &y) {
    const uint32_t a = x, b = y;
    x = (a & cl) | ((b & cl) << s);
    y = ((a & ch) >> s) | (b & ch);
}
// q[2 col + blk] = column col of block blk (little-endian word of its four
// bytes)  <->  the bit planes described above.  Its own inverse.
GCM_HD void ortho(uint32_t q[8]) {
    swapn(0x55555555u, 0xAAAAAAAAu, 1, q[0], q[1]);
    swapn(0x55555555u, 0xAAAAAAAAu, 1, q[2], q[3]);
    swapn(0x55555555u, 0xAAAAAAAAu, 1, q[4], q[5]);
    swapn(0x55555555u, 0xAAAAAAAAu, 1, q[6], q[7]);
    swapn(0x33333333u, 0xCCCCCCCCu, 2, q[0], q[2]);
    swapn(0x33333333u, 0xCCCCCCCCu, 2, q[1], q[3]);
    swapn(0x33333333u, 0xCCCCCCCCu, 2, q[4], q[6]);
    swapn(0x33333333u, 0xCCCCCCCCu, 2, q[5], q[7]);
    swapn(0x0F0F0F0Fu, 0xF0F0F0F0u, 4, q[0], q[4]);
    swapn(0x0F0F0F0Fu, 0xF0F0F0F0u, 4, q[1], q[5]);
    swapn(0x0F0F0F0Fu, 0xF0F0F0F0u, 4, q[2], q[6]);
    swapn(0x0F0F0F0Fu, 0xF0F0F0F0u, 4, q[3], q[7]);
}

// c[0 .. 14] (a product's coefficients) reduced mod x^8 + x^4 + x^3 + x + 1
GCM_HD void gf8_reduce(uint32_t c[15], uint32_t r[8]) {
    GCM_UNROLL
    for (int k = 14; k >= 8; --k) {
        c[k - 4] ^= c[k];
        c[k - 5] ^= c[k];
        c[k - 7] ^= c[k];
        c[k - 8] ^= c[k];
    }
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) r[i] = c[i];
}
GCM_HD void gf8_mul(const uint32_t a[8], const uint32_t b[8], uint32_t r[8]) {
    uint32_t c[15];
    GCM_UNROLL
    for (int k = 0; k < 15; ++k) c[k] = 0;
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) {
        GCM_UNROLL
        for (int j = 0; j < 8; ++j) c[i + j] ^= a[i] & b[j];
    }
    gf8_reduce(c, r);
}
GCM_HD void gf8_sq(const uint32_t a[8], uint32_t r[8]) {
    uint32_t c[15];
    GCM_UNROLL
    for (int k = 0; k < 15; ++k) c[k] = 0;
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) c[2 * i] = a[i];
    gf8_reduce(c, r);
}
// SubBytes on the eight planes: x^254, then the affine map with 0x63
GCM_HD void sbox(uint32_t q[8]) {
    uint32_t x2[8], x3[8], x12[8], t[8], u[8];
    gf8_sq(q, x2);
    gf8_mul(x2, q, x3);
    gf8_sq(x3, t);
    gf8_sq(t, x12);
    gf8_mul(x12, x3, t);  // x^15
    gf8_sq(t, u);
    gf8_sq(u, t);
    gf8_sq(t, u);
    gf8_sq(u, t);          // x^240
    gf8_mul(t, x12, u);    // x^252
    gf8_mul(u, x2, t);     // x^254
    GCM_UNROLL
    for (int i = 0; i < 8; ++i)
        u[i] = t[i] ^ t[(i + 4) & 7] ^ t[(i + 5) & 7] ^ t[(i + 6) & 7] ^ t[(i + 7) & 7];
    q[0] = ~u[0];
    q[1] = ~u[1];
    q[2] = u[2];
    q[3] = u[3];
    q[4] = u[4];
    q[5] = ~u[5];
    q[6] = ~u[6];
    q[7] = u[7];
}
GCM_HD void shift_rows(uint32_t q[8]) {
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint32_t x = q[i];
        q[i] = (x & 0x000000FFu) | ((x & 0x0000FC00u) >> 2) | ((x & 0x00000300u) << 6) | ((x & 0x00F00000u) >> 4) |
               ((x & 0x000F0000u) << 4) | ((x & 0xC0000000u) >> 6) | ((x & 0x3F000000u) << 2);
    }
}
GCM_HD void mix_columns(uint32_t q[8]) {
    uint32_t r[8], t[8];
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) {
        r[i] = rotr32(q[i], 8);  // the row below
        t[i] = q[i] ^ r[i];
    }
    q[0] = t[7] ^ r[0] ^ rotr32(t[0], 16);
    q[1] = t[0] ^ t[7] ^ r[1] ^ rotr32(t[1], 16);
    q[2] = t[1] ^ r[2] ^ rotr32(t[2], 16);
    q[3] = t[2] ^ t[7] ^ r[3] ^ rotr32(t[3], 16);
    q[4] = t[3] ^ t[7] ^ r[4] ^ rotr32(t[4], 16);
    q[5] = t[4] ^ r[5] ^ rotr32(t[5], 16);
    q[6] = t[5] ^ r[6] ^ rotr32(t[6], 16);
    q[7] = t[6] ^ r[7] ^ rotr32(t[7], 16);
}
// E_K of two blocks: q[2 col + blk] in and out, rk the bitsliced round keys
// (read by round index only)
GCM_HD void aes256_encrypt2(const uint32_t *rk, uint32_t q[8]) {
    ortho(q);
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) q[i] ^= rk[i];
    GCM_ROLLED
    for (int r = 1; r < 14; ++r) {
        sbox(q);
        shift_rows(q);
        mix_columns(q);
        GCM_UNROLL
        for (int i = 0; i < 8; ++i) q[i] ^= rk[8 * r + i];
    }
    sbox(q);
    shift_rows(q);
    GCM_UNROLL
    for (int i = 0; i < 8; ++i) q[i] ^= rk[8 * 14 + i];
    ortho(q);
}
GCM_HD uint32_t sub_word(uint32_t x) {
    uint32_t q[8] = {x, 0, 0, 0, 0, 0, 0, 0};
    ortho(q);
    sbox(q);
    ortho(q);
    return q[0];
}
// FIPS-197 key expansion of a 32-byte key into w[60] (little-endian words of
// the schedule's bytes) and the bitsliced round keys rk[RK_WORDS].
GCM_HD void aes256_expand(const uint8_t key[32], uint32_t *w, uint32_t *rk) {
    GCM_ROLLED
    for (int i = 0; i < 8; ++i)
        w[i] = uint32_t(key[4 * i]) | uint32_t(key[4 * i + 1]) << 8 | uint32_t(key[4 * i + 2]) << 16 |
               uint32_t(key[4 * i + 3]) << 24;
    uint32_t rcon = 1;
    GCM_ROLLED
    for (int i = 8; i < 60; ++i) {
        uint32_t t = w[i - 1];
        if ((i & 7) == 0) {
            t = sub_word(rotr32(t, 8)) ^ rcon;
            rcon <<= 1;
        } else if ((i & 7) == 4) {
            t = sub_word(t);
        }
        w[i] = w[i - 8] ^ t;
    }
    GCM_ROLLED
    for (int r = 0; r < 15; ++r) {
        uint32_t q[8];
        GCM_UNROLL
        for (int c = 0; c < 4; ++c) q[2 * c] = q[2 * c + 1] = w[4 * r + c];
        ortho(q);
        GCM_UNROLL
        for (int i = 0; i < 8; ++i) rk[8 * r + i] = q[i];
    }
}
// inc32^(i + 1)(J0): the counter block of real block i; the increment wraps
// in the low 32 bits (the last four bytes, big-endian) only
GCM_HD void counter_block(const uint32_t j0[4], uint64_t i, uint32_t out[4]) {
    out[0] = j0[0];
    out[1] = j0[1];
    out[2] = j0[2];
    out[3] = bswap32(bswap32(j0[3]) + uint32_t(i) + 1u);
}

// ---- blocks at byte-granular addresses ---------------------------------------
// n (1 .. 16) bytes at p as four little-endian words, zero past n.  A whole
// block off a 4-byte boundary is taken from the five aligned words that hold
// it (every one of them has a byte of the block).
GCM_HD void load_block(const uint8_t *p, uint32_t n, uint32_t c[4]) {
    const uint32_t r = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
    if (n == 16 && r == 0) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
        c[0] = q[0];
        c[1] = q[1];
        c[2] = q[2];
        c[3] = q[3];
        return;
    }
    if (n == 16) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - r);
        const uint32_t lo = 8 * r, hi = 32 - lo;
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];
        c[0] = (a0 >> lo) | (a1 << hi);
        c[1] = (a1 >> lo) | (a2 << hi);
        c[2] = (a2 >> lo) | (a3 << hi);
        c[3] = (a3 >> lo) | (a4 << hi);
        return;
    }
    c[0] = c[1] = c[2] = c[3] = 0;
    GCM_UNROLL
    for (uint32_t k = 0; k < 16; ++k)
        if (k < n) c[k >> 2] |= uint32_t(p[k]) << (8 * (k & 3));
}
// the first n (1 .. 16) bytes of c to p and no other byte: a whole block off a
// 4-byte boundary as head bytes, three shifted aligned words and tail bytes
GCM_HD void store_block(uint8_t *p, const uint32_t c[4], uint32_t n) {
    const uint32_t r = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
    if (n == 16 && r == 0) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
        q[0] = c[0];
        q[1] = c[1];
        q[2] = c[2];
        q[3] = c[3];
        return;
    }
    if (n == 16) {
        const uint32_t h = 4 - r, lo = 8 * h, hi = 32 - lo;
        GCM_UNROLL
        for (uint32_t k = 0; k < 3; ++k)
            if (k < h) p[k] = uint8_t(c[0] >> (8 * k));
        uint32_t *q = reinterpret_cast<uint32_t *>(p + h);
        q[0] = (c[0] >> lo) | (c[1] << hi);
        q[1] = (c[1] >> lo) | (c[2] << hi);
        q[2] = (c[2] >> lo) | (c[3] << hi);
        GCM_UNROLL
        for (uint32_t k = 0; k < 3; ++k)
            if (k < r) p[h + 12 + k] = uint8_t(c[3] >> (lo + 8 * k));
        return;
    }
    GCM_UNROLL
    for (uint32_t k = 0; k < 16; ++k)
        if (k < n) p[k] = uint8_t(c[k >> 2] >> (8 * (k & 3)));
}
GCM_HD void mask_block(uint32_t c[4], uint32_t n) {  // zero past the first n (1 .. 16) bytes
    GCM_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t have = n > 4 * j ? n - 4 * j : 0;  // bytes of word j kept
        c[j] &= have >= 4 ? 0xFFFFFFFFu : ((1u << (8 * have)) - 1u);
    }
}

// ---- geometry ------------------------------------------------------------------
GCM_HD uint64_t blocks_of(uint64_t len) { return (len + 15) / 16; }
GCM_HD uint64_t items_of(uint64_t len) { return (blocks_of(len) + SPAN - 1) / SPAN; }

// ---- key setup: one wave per message -------------------------------------------
// a^e for a public exponent e < 128, also returning a^64 (square and multiply;
// the branch is on the exponent's bits only)
GCM_HD B128 gf128_pow_small(const B128 &a, uint32_t e, B128 *a64) {
    B128 r = gf128_one(), p = a;
    GCM_ROLLED
    for (int k = 0; k < 6; ++k) {
        const B128 rp = gf128_mul(r, p);
        if ((e >> k) & 1u) r = rp;
        p = gf128_mul(p, p);
    }
    *a64 = p;
    if (e & 64u) r = gf128_mul(r, p);
    return r;
}
// Lane `lane` of the setup wave: rk is the message's expanded key (already in
// place, read uniformly); writes hp[lane], gp[lane] and, lane 0, the shared
// values.  Every lane computes H for itself: no lane reads another's secrets.
GCM_HD void setup_lane(const uint32_t *rk, const uint8_t iv[16], uint32_t lane, KeyMat *km) {
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    aes256_encrypt2(rk, q);
    const uint32_t hle[4] = {q[0], q[2], q[4], q[6]};
    const B128 H = gf128_from_le(hle);
    B128 h64, g64;
    km->hp[lane] = gf128_pow_small(H, lane, &h64);
    B128 G = gf128_mul(h64, h64);  // H^128
    G = gf128_mul(G, G);           // H^256
    G = gf128_mul(G, G);           // H^512 = H^SPAN
    km->gp[lane] = gf128_pow_small(G, lane, &g64);
    if (lane != 0) return;
    km->hp[LANES] = h64;
    km->gp[LANES] = g64;
    // J0 = GHASH_H(IV || 0^64 || [128]_64)
    uint32_t ivle[4];
    GCM_UNROLL
    for (int c = 0; c < 4; ++c)
        ivle[c] = uint32_t(iv[4 * c]) | uint32_t(iv[4 * c + 1]) << 8 | uint32_t(iv[4 * c + 2]) << 16 |
                  uint32_t(iv[4 * c + 3]) << 24;
    B128 y = gf128_mul(gf128_from_le(ivle), H);
    y.w[3] ^= 128u;
    y = gf128_mul(y, H);
    uint32_t j0[4] = {bswap32(y.w[0]), bswap32(y.w[1]), bswap32(y.w[2]), bswap32(y.w[3])};
    GCM_UNROLL
    for (int c = 0; c < 4; ++c) km->j0[c] = j0[c];
    uint32_t e[8] = {j0[0], 0, j0[1], 0, j0[2], 0, j0[3], 0};
    aes256_encrypt2(rk, e);
    GCM_UNROLL
    for (int c = 0; c < 4; ++c) km->ej0[c] = e[2 * c];
}

// ---- one lane of one item --------------------------------------------------------
// MODE_SEAL: in = plaintext (16-B aligned base), out = ciphertext, absorbs the
//            ciphertext.
// MODE_HASH: in = ciphertext, absorbs it, writes nothing.
// MODE_CTR:  in = ciphertext, out = plaintext when ok, zeros when not;
//            returns zero.
// Returns the lane's share of the item's value (to be XORed over the lanes).
template <uint32_t MODE>
GCM_HD B128 span_lane(const KeyMat *km, const Msg &m, uint32_t item, uint32_t lane, const uint8_t *in, uint8_t *out,
                      bool ok) {
    const uint64_t nb = blocks_of(m.len);
    const uint64_t Z = uint64_t(m.nitems) * SPAN - nb;
    const uint64_t v0 = uint64_t(item) * SPAN + lane;
    B128 acc{{0, 0, 0, 0}};
    const B128 h64 = km->hp[LANES];
    GCM_ROLLED
    for (uint32_t t = 0; t < RUN; t += 2) {
        const uint64_t va = v0 + uint64_t(LANES) * t, vb = va + LANES;
        const bool ha = va >= Z, hb = vb >= Z;  // (vb >= va: ha implies hb)
        const uint64_t ia = va - Z, ib = vb - Z;
        uint32_t ca[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0};
        const uint32_t na = ha ? uint32_t(m.len - 16 * ia < 16 ? m.len - 16 * ia : 16) : 0;
        const uint32_t nbb = hb ? uint32_t(m.len - 16 * ib < 16 ? m.len - 16 * ib : 16) : 0;
        if (MODE == MODE_CTR && !ok) {
            if (ha) store_block(out + 16 * ia, ca, na);
            if (hb) store_block(out + 16 * ib, cb, nbb);
            continue;
        }
        if (!hb) continue;  // leading absent blocks: the state stays zero
        if (ha) load_block(in + 16 * ia, na, ca);
        load_block(in + 16 * ib, nbb, cb);
        if (MODE != MODE_HASH) {
            uint32_t ka[4], kb[4];
            counter_block(km->j0, ia, ka);  // (unused when !ha)
            counter_block(km->j0, ib, kb);
            uint32_t q[8] = {ka[0], kb[0], ka[1], kb[1], ka[2], kb[2], ka[3], kb[3]};
            aes256_encrypt2(km->rk, q);
            GCM_UNROLL
            for (int c = 0; c < 4; ++c) {
                ca[c] ^= q[2 * c];
                cb[c] ^= q[2 * c + 1];
            }
            if (ha) store_block(out + 16 * ia, ca, na);
            store_block(out + 16 * ib, cb, nbb);
            if (ha) mask_block(ca, na);
            mask_block(cb, nbb);
            if (!ha) ca[0] = ca[1] = ca[2] = ca[3] = 0;
        }
        if (MODE != MODE_CTR) {  // Horner with H^64: sum_t X_t H^(64 (RUN - 1 - t))
            acc = gf128_xor(gf128_mul(acc, h64), gf128_from_le(ca));
            acc = gf128_xor(gf128_mul(acc, h64), gf128_from_le(cb));
        }
    }
    if (MODE == MODE_CTR) return acc;
    return gf128_mul(acc, km->hp[LANES - lane]);  // block 64 t + lane of the item gets H^(SPAN - 64 t - lane)
}

// ---- the message's state from its items' values: one wave per message -------------
// Lane `lane`'s share of sum_s V_s G^(nitems - 1 - s) (XOR over the lanes).
GCM_HD B128 finish_lane(const KeyMat *km, const B128 *vals, uint32_t nitems, uint32_t lane) {
    const uint32_t steps = (nitems + LANES - 1) / LANES;
    const uint32_t Z = steps * LANES - nitems;
    const B128 g64 = km->gp[LANES];
    B128 acc{{0, 0, 0, 0}};
    GCM_ROLLED
    for (uint32_t t = 0; t < steps; ++t) {
        const uint32_t v = t * LANES + lane;
        acc = gf128_mul(acc, g64);
        if (v >= Z) acc = gf128_xor(acc, vals[v - Z]);
    }
    return gf128_mul(acc, km->gp[LANES - 1 - lane]);
}
// tag = E_K(J0) ^ (state ^ [0]_64 [8 len]_64) H, as four little-endian words
GCM_HD void final_tag(const KeyMat *km, const B128 &state, uint64_t len, uint32_t tag[4]) {
    B128 y = state;
    const uint64_t bits = len * 8;
    y.w[2] ^= uint32_t(bits >> 32);
    y.w[3] ^= uint32_t(bits);
    y = gf128_mul(y, km->hp[1]);
    GCM_UNROLL
    for (int c = 0; c < 4; ++c) tag[c] = bswap32(y.w[c]) ^ km->ej0[c];
}

}  // namespace gcm
}  // namespace chip
