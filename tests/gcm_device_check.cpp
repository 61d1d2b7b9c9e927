// gcm_device_check.cpp — stand-alone check of carbonado_amd/csrc/gcm_device.hpp
// and ecies_plan.hpp, compiled for the host under ASan + UBSan and linked with
// libcrypto (tests/test_ecies_dev_cpu.py builds and runs it):
//   - the S-box circuit against the FIPS-197 table, all 256 inputs in every
//     one of the 32 bit positions of the planes;
//   - the FIPS-197 C.3 AES-256 vector, in both block positions;
//   - gf128_mul against a plain bit-loop restatement on random pairs, and the
//     identities with 0, 1 and x^127;
//   - the counter block for a J0 whose low word is 0xFFFFFFFE, blocks 0 to 3;
//   - load_block / store_block at every residue and length, no byte beside;
//   - a whole-message walk that splits the work exactly as the kernels do
//     (setup_lane per lane, span_lane per item and lane, finish_lane per lane,
//     final_tag) against EVP AES-256-GCM with a 16-byte IV, seal and open, at
//     every partition boundary the kernels have, +-1;
//   - ecies_plan.hpp: disjoint scratch regions, the key region covered by the
//     wipe, offsets, and the argument checks.
#include <openssl/evp.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/ecies_plan.hpp"

using namespace chip;
using namespace chip::gcm;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            ++failures;                                           \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                         \
    } while (0)

static const uint8_t SBOX[256] = {
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76, 0xca, 0x82, 0xc9,
    0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0, 0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f,
    0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15, 0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07,
    0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75, 0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3,
    0x29, 0xe3, 0x2f, 0x84, 0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58,
    0xcf, 0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8, 0x51, 0xa3,
    0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2, 0xcd, 0x0c, 0x13, 0xec, 0x5f,
    0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73, 0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88,
    0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb, 0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac,
    0x62, 0x91, 0x95, 0xe4, 0x79, 0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a,
    0xae, 0x08, 0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a, 0x70,
    0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e, 0xe1, 0xf8, 0x98, 0x11,
    0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf, 0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42,
    0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16};

static void check_sbox() {
    // the byte x at bit position pos of the planes, every other position holding x + pos + other
    for (int pos = 0; pos < 32; ++pos)
        for (int x = 0; x < 256; ++x) {
            uint8_t bytes[32];
            for (int p = 0; p < 32; ++p) bytes[p] = uint8_t(p == pos ? x : x * 7 + p * 13 + pos);
            uint32_t q[8] = {};
            for (int p = 0; p < 32; ++p)
                for (int b = 0; b < 8; ++b) q[b] |= uint32_t((bytes[p] >> b) & 1) << p;
            sbox(q);
            bool ok = true;
            for (int p = 0; p < 32; ++p) {
                uint8_t y = 0;
                for (int b = 0; b < 8; ++b) y |= uint8_t(((q[b] >> p) & 1) << b);
                ok &= y == SBOX[bytes[p]];
            }
            CHECK(ok);
        }
}

static void check_fips_c3() {
    uint8_t key[32], pt[16];
    for (int i = 0; i < 32; ++i) key[i] = uint8_t(i);
    for (int i = 0; i < 16; ++i) pt[i] = uint8_t(i * 0x11);
    static const uint8_t want[16] = {0x8e, 0xa2, 0xb7, 0xca, 0x51, 0x67, 0x45, 0xbf,
                                     0xea, 0xfc, 0x49, 0x90, 0x4b, 0x49, 0x60, 0x89};
    uint32_t w[60], rk[RK_WORDS];
    aes256_expand(key, w, rk);
    uint32_t c[4];
    load_block(pt, 16, c);
    for (int pos = 0; pos < 2; ++pos) {
        uint32_t q[8] = {};
        for (int k = 0; k < 4; ++k) {
            q[2 * k + pos] = c[k];
            q[2 * k + 1 - pos] = 0x01020304u * (k + 1);
        }
        aes256_encrypt2(rk, q);
        uint8_t got[16];
        const uint32_t o[4] = {q[pos], q[2 + pos], q[4 + pos], q[6 + pos]};
        store_block(got, o, 16);
        CHECK(std::memcmp(got, want, 16) == 0);
    }
    // the other block of the pair against EVP (ECB)
    EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
    std::mt19937_64 rng(7);
    for (int it = 0; it < 50; ++it) {
        uint8_t k2[32], in[32], ref[48];
        for (auto &b : k2) b = uint8_t(rng());
        for (auto &b : in) b = uint8_t(rng());
        int n = 0;
        EVP_EncryptInit_ex(ctx, EVP_aes_256_ecb(), nullptr, k2, nullptr);
        EVP_CIPHER_CTX_set_padding(ctx, 0);
        EVP_EncryptUpdate(ctx, ref, &n, in, 32);
        aes256_expand(k2, w, rk);
        uint32_t a[4], b[4];
        load_block(in, 16, a);
        load_block(in + 16, 16, b);
        uint32_t q[8] = {a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3]};
        aes256_encrypt2(rk, q);
        uint8_t got[32];
        const uint32_t oa[4] = {q[0], q[2], q[4], q[6]}, ob[4] = {q[1], q[3], q[5], q[7]};
        store_block(got, oa, 16);
        store_block(got + 16, ob, 16);
        CHECK(std::memcmp(got, ref, 32) == 0);
    }
    EVP_CIPHER_CTX_free(ctx);
}

// NIST SP 800-38D algorithm 1, bit by bit on byte arrays
static void ref_gf128_mul(const uint8_t x[16], const uint8_t y[16], uint8_t z[16]) {
    uint8_t v[16];
    std::memcpy(v, y, 16);
    std::memset(z, 0, 16);
    for (int i = 0; i < 128; ++i) {
        if ((x[i / 8] >> (7 - i % 8)) & 1)
            for (int k = 0; k < 16; ++k) z[k] ^= v[k];
        const int lsb = v[15] & 1;
        for (int k = 15; k > 0; --k) v[k] = uint8_t((v[k] >> 1) | (v[k - 1] << 7));
        v[0] >>= 1;
        if (lsb) v[0] ^= 0xE1;
    }
}
static B128 from_bytes(const uint8_t b[16]) {
    B128 r;
    for (int j = 0; j < 4; ++j)
        r.w[j] = uint32_t(b[4 * j]) << 24 | uint32_t(b[4 * j + 1]) << 16 | uint32_t(b[4 * j + 2]) << 8 | b[4 * j + 3];
    return r;
}
static bool eq(const B128 &a, const B128 &b) { return std::memcmp(a.w, b.w, 16) == 0; }

static void check_gf128() {
    std::mt19937_64 rng(11);
    for (int it = 0; it < 2000; ++it) {
        uint8_t x[16], y[16], z[16];
        for (auto &b : x) b = uint8_t(rng());
        for (auto &b : y) b = uint8_t(rng());
        ref_gf128_mul(x, y, z);
        CHECK(eq(gf128_mul(from_bytes(x), from_bytes(y)), from_bytes(z)));
        const B128 a = from_bytes(x), zero{{0, 0, 0, 0}};
        CHECK(eq(gf128_mul(a, zero), zero) && eq(gf128_mul(zero, a), zero));
        CHECK(eq(gf128_mul(a, gf128_one()), a) && eq(gf128_mul(gf128_one(), a), a));
        // a x^127: the bit loop restated for that one operand
        uint8_t x127[16] = {};
        x127[15] = 1;
        ref_gf128_mul(x, x127, z);
        const B128 top{{0, 0, 0, 1}};
        CHECK(eq(gf128_mul(a, top), from_bytes(z)) && eq(gf128_mul(top, a), from_bytes(z)));
    }
    // x^127 * x = the reduction polynomial's low part
    const B128 top{{0, 0, 0, 1}}, x1{{0x40000000u, 0, 0, 0}}, red{{0xE1000000u, 0, 0, 0}};
    CHECK(eq(gf128_mul(top, x1), red));
    // small powers: a^e against repeated multiplication
    uint8_t hb[16];
    for (auto &b : hb) b = uint8_t(rng());
    const B128 h = from_bytes(hb);
    B128 p = gf128_one();
    for (uint32_t e = 0; e <= 64; ++e) {
        B128 h64;
        CHECK(eq(gf128_pow_small(h, e, &h64), p));
        p = gf128_mul(p, h);
    }
}

static void check_counter() {
    const uint8_t j0b[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0xFF, 0xFF, 0xFF, 0xFE};
    uint32_t j0[4];
    load_block(j0b, 16, j0);
    const uint32_t low[4] = {0xFFFFFFFFu, 0x00000000u, 0x00000001u, 0x00000002u};
    for (int i = 0; i < 4; ++i) {
        uint32_t c[4];
        counter_block(j0, uint64_t(i), c);
        uint8_t out[16];
        store_block(out, c, 16);
        CHECK(std::memcmp(out, j0b, 12) == 0);
        CHECK((uint32_t(out[12]) << 24 | uint32_t(out[13]) << 16 | uint32_t(out[14]) << 8 | out[15]) == low[i]);
    }
}

static void check_edges() {
    alignas(16) uint8_t buf[96], src[96];
    for (int i = 0; i < 96; ++i) src[i] = uint8_t(i * 3 + 1);
    for (uint32_t r = 0; r < 16; ++r)
        for (uint32_t n = 1; n <= 16; ++n) {
            uint32_t c[4];
            load_block(src + 32 + r, n, c);
            uint8_t flat[16];
            for (int k = 0; k < 16; ++k) flat[k] = uint8_t(c[k >> 2] >> (8 * (k & 3)));
            bool ok = true;
            for (uint32_t k = 0; k < 16; ++k) ok &= flat[k] == (k < n ? src[32 + r + k] : 0);
            CHECK(ok);
            std::memset(buf, 0xA5, sizeof buf);
            uint32_t full[4];
            load_block(src + 16, 16, full);
            store_block(buf + 32 + r, full, n);
            for (uint32_t k = 0; k < 96; ++k) {
                const bool in = k >= 32 + r && k < 32 + r + n;
                ok &= buf[k] == (in ? src[16 + k - 32 - r] : 0xA5);
            }
            CHECK(ok);
            uint32_t m[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            mask_block(m, n);
            for (uint32_t k = 0; k < 16; ++k) ok &= uint8_t(m[k >> 2] >> (8 * (k & 3))) == (k < n ? 0xFF : 0);
            CHECK(ok);
        }
}

// ---- the whole message, split as the kernels split it --------------------------
struct Walk {
    KeyMat km;
    Msg m;
};
static void walk_setup(Walk &w, const uint8_t key[32], const uint8_t iv[16], uint64_t len) {
    uint32_t sched[60];
    std::memset(&w.km, 0, sizeof w.km);
    aes256_expand(key, sched, w.km.rk);
    for (uint32_t lane = 0; lane < LANES; ++lane) setup_lane(w.km.rk, iv, lane, &w.km);
    w.m = Msg{};
    w.m.len = len;
    w.m.nitems = uint32_t(items_of(len));
}
template <uint32_t MODE>
static void walk_items(const Walk &w, const uint8_t *in, uint8_t *out, bool ok, std::vector<B128> *vals) {
    vals->assign(w.m.nitems, B128{{0, 0, 0, 0}});
    for (uint32_t s = 0; s < w.m.nitems; ++s)
        for (uint32_t lane = 0; lane < LANES; ++lane)
            (*vals)[s] = gf128_xor((*vals)[s], span_lane<MODE>(&w.km, w.m, s, lane, in, out, ok));
}
static void walk_tag(const Walk &w, const std::vector<B128> &vals, uint8_t tag[16]) {
    B128 st{{0, 0, 0, 0}};
    for (uint32_t lane = 0; lane < LANES; ++lane)
        st = gf128_xor(st, finish_lane(&w.km, vals.data(), w.m.nitems, lane));
    uint32_t t[4];
    final_tag(&w.km, st, w.m.len, t);
    store_block(tag, t, 16);
}

static void evp_seal(const uint8_t key[32], const uint8_t iv[16], const uint8_t *pt, size_t n, uint8_t *ct,
                     uint8_t tag[16]) {
    EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
    int len = 0;
    EVP_EncryptInit_ex(ctx, EVP_aes_256_gcm(), nullptr, nullptr, nullptr);
    EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, 16, nullptr);
    EVP_EncryptInit_ex(ctx, nullptr, nullptr, key, iv);
    uint8_t dummy[16];
    if (n) EVP_EncryptUpdate(ctx, ct, &len, pt, int(n));
    EVP_EncryptFinal_ex(ctx, n ? ct + len : dummy, &len);
    EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag);
    EVP_CIPHER_CTX_free(ctx);
}

static void check_message(std::mt19937_64 &rng, uint64_t len, uint32_t residue, const uint8_t *fixed_key = nullptr,
                          const uint8_t *fixed_iv = nullptr) {
    uint8_t key[32], iv[16];
    for (auto &b : key) b = uint8_t(rng());
    for (auto &b : iv) b = uint8_t(rng());
    if (fixed_key) std::memcpy(key, fixed_key, 32);
    if (fixed_iv) std::memcpy(iv, fixed_iv, 16);
    // slack on both sides: a block off a word boundary is moved in aligned words
    std::vector<uint8_t> ptbuf(len + 64), ctbuf(len + 64, 0xC3), ref(len + 16), back(len + 64, 0x5A);
    uint8_t *pt = ptbuf.data() + 32 - (reinterpret_cast<uintptr_t>(ptbuf.data()) & 15);
    uint8_t *ct = ctbuf.data() + 32 - (reinterpret_cast<uintptr_t>(ctbuf.data()) & 15) + residue;
    uint8_t *pl = back.data() + 32 - (reinterpret_cast<uintptr_t>(back.data()) & 15);
    for (uint64_t i = 0; i < len; ++i) pt[i] = uint8_t(rng());
    uint8_t rtag[16], tag[16];
    evp_seal(key, iv, pt, len, ref.data(), rtag);
    Walk w;
    walk_setup(w, key, iv, len);
    std::vector<B128> vals;
    walk_items<MODE_SEAL>(w, pt, ct, true, &vals);
    walk_tag(w, vals, tag);
    CHECK(std::memcmp(tag, rtag, 16) == 0);
    CHECK(len == 0 || std::memcmp(ct, ref.data(), len) == 0);
    bool clean = true;
    for (uint8_t *p = ctbuf.data(); p < ctbuf.data() + ctbuf.size(); ++p)
        if (p < ct || p >= ct + len) clean &= *p == 0xC3;
    CHECK(clean);
    // open: hash, then the gated pass
    walk_items<MODE_HASH>(w, ct, nullptr, true, &vals);
    walk_tag(w, vals, tag);
    CHECK(std::memcmp(tag, rtag, 16) == 0);
    std::vector<B128> none;
    walk_items<MODE_CTR>(w, ct, pl, true, &none);
    CHECK(len == 0 || std::memcmp(pl, pt, len) == 0);
    walk_items<MODE_CTR>(w, ct, pl, false, &none);
    clean = true;
    for (uint8_t *p = back.data(); p < back.data() + back.size(); ++p)
        clean &= *p == ((p >= pl && p < pl + len) ? 0 : 0x5A);
    CHECK(clean);
    if (len) {  // a flipped ciphertext bit changes the tag
        ct[len / 2] ^= 0x10;
        walk_items<MODE_HASH>(w, ct, nullptr, true, &vals);
        walk_tag(w, vals, tag);
        CHECK(std::memcmp(tag, rtag, 16) != 0);
    }
}

static void check_plan() {
    std::mt19937_64 rng(5);
    for (int it = 0; it < 200; ++it) {
        const uint64_t count = 1 + rng() % 40;
        std::vector<uint64_t> len(count), in_off(count), out_off(count);
        uint64_t ip = 0, op = 0, items = 0;
        for (uint64_t o = 0; o < count; ++o) {
            len[o] = (rng() % 4 == 0) ? 0 : rng() % 70000;
            in_off[o] = ip;
            ip += (len[o] + 15) / 16 * 16 + 16 * (rng() % 3);
            out_off[o] = op + rng() % 16;
            op = out_off[o] + len[o] + rng() % 5;
            items += items_of(len[o]);
        }
        std::vector<uint8_t> keys(32 * count), ivs(16 * count);
        for (auto &b : keys) b = uint8_t(rng());
        for (auto &b : ivs) b = uint8_t(rng());
        const uint64_t need = ecies::gcm_scratch_len(len.data(), count);
        const ecies::Layout l = ecies::layout(count, items);
        CHECK(need == l.total && need % 16 == 0);
        // regions in order, disjoint, aligned, inside the length; the key region is what the wipe covers
        CHECK(l.msgs == 0 && l.msgs + count * sizeof(Msg) <= l.hdrs && l.hdrs + 96 * count == l.keys && l.keys + 48 * count == l.km);
        CHECK(l.km + count * sizeof(KeyMat) == l.vals && l.vals + 16 * items == l.ok && l.ok + 4 * count <= l.total);
        CHECK(l.hdrs % 16 == 0 && l.keys % 16 == 0 && l.km % 16 == 0 && l.vals % 16 == 0 && l.ok % 16 == 0);
        CHECK(l.wipe_from() == l.keys && l.wipe_from() + l.wipe_len() == l.ok && l.upload_len() == l.km);
        ecies::Plan p;
        const uintptr_t D = 0x10000000, OUT = 0x30000000, TAG = 0x50000000, SCR = 0x70000000;
        CHECK(ecies::plan_gcm(true, keys.data(), ivs.data(), D, in_off.data(), len.data(), count, OUT, out_off.data(),
                              TAG, nullptr, true, SCR, need, &p) == CHIP_OK);
        CHECK(p.items == items && p.table.size() == l.upload_len());
        uint64_t i0 = 0;
        for (uint64_t o = 0; o < count; ++o) {
            Msg m;
            std::memcpy(&m, p.table.data() + o * sizeof(Msg), sizeof m);
            CHECK(m.in_off == in_off[o] && m.out_off == out_off[o] && m.tag_off == 16 * o && m.len == len[o]);
            CHECK(m.item0 == i0 && m.nitems == items_of(len[o]));
            i0 += m.nitems;
            CHECK(std::memcmp(p.table.data() + l.keys + 48 * o, keys.data() + 32 * o, 32) == 0);
            CHECK(std::memcmp(p.table.data() + l.keys + 48 * o + 32, ivs.data() + 16 * o, 16) == 0);
        }
        CHECK(ecies::plan_gcm(true, keys.data(), ivs.data(), D, in_off.data(), len.data(), count, OUT, out_off.data(),
                              TAG, nullptr, true, SCR, need - 1, &p) == CHIP_ERR_INVALID_ARG);
        CHECK(ecies::plan_gcm(true, keys.data(), ivs.data(), D, in_off.data(), len.data(), count, OUT, out_off.data(),
                              TAG, nullptr, true, SCR + 8, need, &p) == CHIP_ERR_INVALID_ARG);
        if (count >= 2 && len[0] && len[1]) {
            std::vector<uint64_t> bad = out_off;
            bad[1] = bad[0] + len[0] - 1;
            CHECK(ecies::plan_gcm(true, keys.data(), ivs.data(), D, in_off.data(), len.data(), count, OUT, bad.data(),
                                  TAG, nullptr, true, SCR, need, &p) == CHIP_ERR_INVALID_ARG);
        }
    }
    CHECK(items_of(0) == 0 && items_of(1) == 1 && items_of(8192) == 1 && items_of(8193) == 2);
    CHECK(sizeof(KeyMat) % 16 == 0 && sizeof(Msg) == 48);
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
    const bool big = argc > 2 && std::strcmp(argv[2], "big") == 0;
    std::mt19937_64 rng(seed);
    if (!big) {
        check_sbox();
        check_fips_c3();
        check_gf128();
        check_counter();
        check_edges();
        check_plan();
        // block, pair of blocks, a wave's row of 64 blocks, an item, two items
        const uint64_t lens[] = {0,    1,    15,   16,   17,   31,   32,    33,    1023, 1024,
                                 1025, 2047, 2048, 2049, 8191, 8192, 8193,  16383, 16384, 16385};
        uint32_t k = 0;
        for (uint64_t len : lens) check_message(rng, len, (k++ * 5 + 1) % 16);
        for (uint32_t r = 0; r < 16; ++r) check_message(rng, 100 + r, r);
    } else {
        // 64 items: the boundary of the second level's lanes and of its Horner step
        const uint64_t edge = uint64_t(SPAN) * 16 * LANES;
        check_message(rng, edge - 1, 1);
        check_message(rng, edge, 7);
        check_message(rng, edge + 1, 13);
    }
    std::printf("gcm_device_check seed %llu%s: %d failures\n", (unsigned long long)seed, big ? " big" : "", failures);
    return failures ? 1 : 0;
}
