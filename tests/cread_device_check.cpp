// cread_device_check.cpp — stand-alone check of carbonado_amd/csrc/cread_device.hpp
// and cread_plan.hpp, compiled for the host under ASan + UBSan and linked with
// libcrypto (tests/test_cread_cpu.py builds and runs it).  It compiles the text
// the kernels of cread_kernels.hip compile and walks every call as they split
// it: the plan's table, setup_lite per key, then per work item lane_eval for
// the 64 lanes, the neighbour exchange (lane l takes lane l + 1's first block;
// lane 63 gets poison, which it must not look at) and lane_apply, on a buffer
// whose last item ends at the allocation's last byte.  Compared with EVP
// AES-256-GCM (16-byte IV) ciphertext ^ plaintext:
//   - every pos % 16 times the lengths {0, 1, 15, 16, 17, 31, 32, 33} and the
//     lengths around one and two spans, +-1;
//   - positions around 8192, +-1;
//   - setup_lite's J0 against its definition (H from EVP ECB, GHASH by a bit
//     loop);
//   - the committed counter-wrap pair: a range across block 2^32 - 1 - J0's low
//     word, and one that starts at the block behind it;
//   - killed items (zeros, nothing beside), the plan's regions and its checks.
#include <openssl/evp.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/cread_plan.hpp"

using namespace chip;
using namespace chip::cread;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            ++failures;                                           \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                         \
    } while (0)

static std::vector<uint8_t> evp_gcm(const uint8_t key[32], const uint8_t iv[16], const std::vector<uint8_t> &pt) {
    std::vector<uint8_t> ct(pt.size() + 16);
    EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
    int n = 0;
    EVP_EncryptInit_ex(ctx, EVP_aes_256_gcm(), nullptr, nullptr, nullptr);
    EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, 16, nullptr);
    EVP_EncryptInit_ex(ctx, nullptr, nullptr, key, iv);
    if (!pt.empty()) EVP_EncryptUpdate(ctx, ct.data(), &n, pt.data(), int(pt.size()));
    CHECK(size_t(n) == pt.size());
    EVP_CIPHER_CTX_free(ctx);
    ct.resize(pt.size());
    return ct;
}

static void evp_ecb(const uint8_t key[32], const uint8_t in[16], uint8_t out[16]) {
    EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
    uint8_t buf[32];
    int n = 0;
    EVP_EncryptInit_ex(ctx, EVP_aes_256_ecb(), nullptr, key, nullptr);
    EVP_CIPHER_CTX_set_padding(ctx, 0);
    EVP_EncryptUpdate(ctx, buf, &n, in, 16);
    EVP_CIPHER_CTX_free(ctx);
    std::memcpy(out, buf, 16);
}

// NIST SP 800-38D algorithm 1, bit by bit on byte arrays
static void ref_gf128_mul(const uint8_t x[16], const uint8_t y[16], uint8_t z[16]) {
    uint8_t v[16], r[16] = {};
    std::memcpy(v, y, 16);
    for (int i = 0; i < 128; ++i) {
        if ((x[i / 8] >> (7 - i % 8)) & 1)
            for (int k = 0; k < 16; ++k) r[k] ^= v[k];
        const int lsb = v[15] & 1;
        for (int k = 15; k > 0; --k) v[k] = uint8_t((v[k] >> 1) | (v[k - 1] << 7));
        v[0] >>= 1;
        if (lsb) v[0] ^= 0xE1;
    }
    std::memcpy(z, r, 16);
}

static void ref_j0(const uint8_t key[32], const uint8_t iv[16], uint8_t j0[16]) {
    uint8_t h[16], zero[16] = {}, y[16];
    evp_ecb(key, zero, h);
    ref_gf128_mul(iv, h, y);
    y[15] ^= 128;
    ref_gf128_mul(y, h, j0);
}

struct Call {
    std::vector<uint8_t> keys, ivs;  // per key
    std::vector<uint32_t> item_key, kill;
    std::vector<uint64_t> pos, n, off;
};

// the call on host memory, split as the kernels split it
static void walk(const Call &c, uint8_t *buf, uint64_t buf_len) {
    const uint64_t nkeys = c.keys.size() / 32, nitems = c.n.size();
    const uint64_t need = scratch_len(nkeys, nitems);
    CHECK(need % 16 == 0 && need > 0);
    alignas(16) static uint8_t anchor[16];
    Plan p;
    const int st = plan_ctr(c.keys.data(), c.ivs.data(), nkeys, c.item_key.data(), c.pos.data(), c.n.data(), nitems,
                            reinterpret_cast<uintptr_t>(buf), c.off.data(), reinterpret_cast<uintptr_t>(anchor), need,
                            c.kill.empty() ? nullptr : c.kill.data(), &p);
    CHECK(st == CHIP_OK);
    if (st != CHIP_OK) return;
    CHECK(p.lay.keys % 16 == 0 && p.lay.km % 16 == 0 && p.lay.total == need && p.table.size() == p.lay.km);
    CHECK(p.lay.wipe_from() == p.lay.keys && p.lay.wipe_from() + p.lay.wipe_len() == p.lay.total);
    const Item *items = reinterpret_cast<const Item *>(p.table.data() + p.lay.items);
    std::vector<CtrKey> km(p.keys_used);
    for (uint32_t k = 0; k < p.keys_used; ++k) {  // the setup kernel
        const uint8_t *raw = p.table.data() + p.lay.keys + 48ull * k;
        uint32_t w[60];
        gcm::aes256_expand(raw, w, km[k].rk);
        setup_lite(km[k].rk, raw + 32, km[k].j0);
    }
    std::vector<uint32_t> status(nitems, 0xC5C5C5C5u), used(status), vouch(status);  // the result words, canaries
    for (uint64_t w = 0; w < p.work; ++w) {  // the range kernel, one wave per work item
        const uint32_t i = item_of(items, uint32_t(nitems), uint32_t(w));
        const Item it = items[i];
        CHECK(w >= it.work0 && w - it.work0 < work_of(it.n, it.kill));
        const uint32_t span = uint32_t(w) - it.work0;
        CHECK(it.buf_off + it.n <= buf_len);
        uint8_t *b = buf + it.buf_off;
        if (it.kill) {
            for (uint32_t l = 0; l < LANES; ++l)
                lane_kill(it, span, l, b, status.data(), used.data(), vouch.data(), i);
            continue;
        }
        uint32_t ka[LANES + 1][4], kb[LANES][4];
        for (uint32_t l = 0; l < LANES; ++l) {
            for (int j = 0; j < 4; ++j) ka[l][j] = kb[l][j] = 0;
            if (lane_needed(it, span, l)) lane_eval(&km[it.key], it, span, l, ka[l], kb[l]);
        }
        for (int j = 0; j < 4; ++j) ka[LANES][j] = 0xDEADBEEFu;  // what lane 63's shuffle reads is not defined
        for (uint32_t l = 0; l < LANES; ++l) lane_apply(it, span, l, ka[l], kb[l], ka[l + 1], b);
    }
    for (uint64_t i = 0; i < nitems; ++i) {  // a killed item's words are its status and zeros, a live one's untouched
        const uint32_t k = items[i].kill;
        CHECK(status[i] == (k ? k : 0xC5C5C5C5u) && used[i] == (k ? 0u : 0xC5C5C5C5u) && vouch[i] == used[i]);
    }
}

struct Msg {
    uint8_t key[32], iv[16];
    std::vector<uint8_t> pt, ct;
};
static Msg make_msg(std::mt19937_64 &rng, uint64_t len, const uint8_t *key = nullptr, const uint8_t *iv = nullptr) {
    Msg m;
    for (auto &b : m.key) b = uint8_t(rng());
    for (auto &b : m.iv) b = uint8_t(rng());
    if (key) std::memcpy(m.key, key, 32);
    if (iv) std::memcpy(m.iv, iv, 16);
    m.pt.resize(len);
    for (auto &b : m.pt) b = uint8_t(rng());
    m.ct = evp_gcm(m.key, m.iv, m.pt);
    return m;
}

// items (key index, pos, n) over messages: the buffer holds ciphertext slices
// at 16-B aligned offsets with canary gaps, the walk must leave plaintext
// slices and every other byte alone; the last item ends the allocation
static void run_items(const std::vector<Msg> &msgs, const std::vector<uint32_t> &mk, const std::vector<uint64_t> &pos,
                      const std::vector<uint64_t> &n, const std::vector<uint32_t> &kill = {}) {
    Call c;
    for (const Msg &m : msgs) {
        c.keys.insert(c.keys.end(), m.key, m.key + 32);
        c.ivs.insert(c.ivs.end(), m.iv, m.iv + 16);
    }
    c.item_key = mk;
    c.pos = pos;
    c.n = n;
    c.kill = kill;
    uint64_t at = 0, end = 0;
    for (size_t i = 0; i < n.size(); ++i) {
        c.off.push_back(at);
        if (n[i]) end = at + n[i];
        at += up16(n[i]) + 16;
    }
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, end ? end : 16) != 0) std::abort();
    uint8_t *buf = static_cast<uint8_t *>(mem);
    std::vector<uint8_t> want(end, 0xC5);
    std::memset(buf, 0xC5, end);
    for (size_t i = 0; i < n.size(); ++i) {
        if (!n[i]) continue;
        const Msg &m = msgs[mk[i]];
        std::memcpy(buf + c.off[i], m.ct.data() + pos[i], n[i]);
        if (!kill.empty() && kill[i]) std::memset(want.data() + c.off[i], 0, n[i]);
        else std::memcpy(want.data() + c.off[i], m.pt.data() + pos[i], n[i]);
    }
    walk(c, buf, end);
    CHECK(std::memcmp(buf, want.data(), end) == 0);
    if (kill.empty()) {  // applied twice it is the identity
        walk(c, buf, end);
        bool same = true;
        for (size_t i = 0; i < n.size(); ++i)
            same &= !n[i] || std::memcmp(buf + c.off[i], msgs[mk[i]].ct.data() + pos[i], n[i]) == 0;
        CHECK(same);
    }
    std::free(mem);
}

static void check_ks_shift() {
    uint8_t ab[32];
    for (int i = 0; i < 32; ++i) ab[i] = uint8_t(0x10 + i);
    uint32_t a[4], b[4];
    gcm::load_block(ab, 16, a);
    gcm::load_block(ab + 16, 16, b);
    for (uint32_t sh = 0; sh < 16; ++sh) {
        uint32_t o[4];
        uint8_t got[16];
        ks_shift(a, b, sh, o);
        gcm::store_block(got, o, 16);
        CHECK(std::memcmp(got, ab + sh, 16) == 0);
    }
}

static void check_j0(std::mt19937_64 &rng) {
    for (int t = 0; t < 8; ++t) {
        uint8_t key[32], iv[16], want[16], got[16];
        for (auto &b : key) b = uint8_t(rng());
        for (auto &b : iv) b = uint8_t(rng());
        ref_j0(key, iv, want);
        uint32_t w[60], rk[gcm::RK_WORDS], j0[4];
        gcm::aes256_expand(key, w, rk);
        setup_lite(rk, iv, j0);
        gcm::store_block(got, j0, 16);
        CHECK(std::memcmp(got, want, 16) == 0);
    }
}

static void check_edges(std::mt19937_64 &rng) {
    const uint64_t S = uint64_t(SPAN_UNITS) * 16;
    std::vector<Msg> msgs;
    msgs.push_back(make_msg(rng, 3 * S + 100));
    msgs.push_back(make_msg(rng, 20000));
    msgs.push_back(make_msg(rng, 100));
    const uint64_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, S - 17, S - 16, S - 15, S - 1, S, S + 1, S + 16, S + 17,
                             2 * S - 1, 2 * S, 2 * S + 1};
    std::vector<uint32_t> mk;
    std::vector<uint64_t> pos, n;
    for (uint64_t sh = 0; sh < 16; ++sh)
        for (uint64_t len : lens) {
            mk.push_back(0);
            pos.push_back(32 + sh);
            n.push_back(len);
        }
    run_items(msgs, mk, pos, n);
    mk.clear(), pos.clear(), n.clear();
    for (uint64_t p : {8191, 8192, 8193})
        for (uint64_t len : {1, 100, 2033}) {
            mk.push_back(1);
            pos.push_back(p);
            n.push_back(len);
        }
    // a whole message, an item that ends at a message's last byte, two items of one key, an unused key in between
    mk.insert(mk.end(), {2, 1, 0, 0});
    pos.insert(pos.end(), {0, 20000 - 77, 0, 3 * S + 100 - 1});
    n.insert(n.end(), {100, 77, 5, 1});
    run_items(msgs, mk, pos, n);
    // killed items among live ones: zeros, one work item even when empty
    std::vector<uint32_t> kill = {0, 17, 7, 0, 5};
    run_items(msgs, {0, 1, 1, 2, 0}, {5, 9, 100, 3, 7}, {40, S + 3, 0, 20, 33}, kill);
}

static void check_wrap(std::mt19937_64 &rng) {
    static const uint8_t KEY[32] = {0xc6, 0x75, 0xbe, 0xa6, 0xd1, 0x50, 0x36, 0x7b, 0x0f, 0xa6, 0xdb, 0xcb, 0x7e, 0x14, 0x25, 0x08,
                                    0x52, 0x82, 0x34, 0x10, 0x3f, 0x6d, 0x17, 0x8e, 0x38, 0xa1, 0xab, 0x87, 0x36, 0x27, 0x0c, 0x09};
    static const uint8_t IV[16] = {0x54, 0x36, 0xaa, 0x02, 0x34, 0x89, 0x64, 0x11, 0x57, 0x5d, 0x56, 0xbb, 0xd2, 0x09, 0x5d, 0xc7};
    uint8_t j0[16];
    ref_j0(KEY, IV, j0);
    const uint32_t low = uint32_t(j0[12]) << 24 | uint32_t(j0[13]) << 16 | uint32_t(j0[14]) << 8 | j0[15];
    const uint64_t istar = 0xFFFFFFFFull - low;  // real block i uses low + i + 1: this one takes the last value before the wrap
    CHECK(istar == 0x85d9 && 16 * (istar + 2) < (1u << 20));
    std::vector<Msg> msgs;
    msgs.push_back(make_msg(rng, 1 << 20, KEY, IV));
    run_items(msgs, {0, 0, 0}, {16 * istar - 41, 16 * (istar + 1), 16 * istar + 100}, {100, 100, 4000});
}

static void check_plan() {
    alignas(16) static uint8_t scr[16];
    const uintptr_t S = reinterpret_cast<uintptr_t>(scr), B = 0x10000;
    const uint8_t keys[64] = {}, ivs[32] = {};
    const uint32_t ik[3] = {0, 1, 0};
    const uint64_t pos[3] = {5, 0, 99}, n[3] = {100, 0, 17}, off[3] = {0, 8, 112};
    const uint64_t need = scratch_len(2, 3);
    Plan p;
    auto rc = [&](const uint8_t *k, uint64_t nitems, const uint32_t *key, const uint64_t *ps, const uint64_t *ns, uintptr_t b,
                  const uint64_t *of, uintptr_t s, uint64_t len) {
        return plan_ctr(k, ivs, 2, key, ps, ns, nitems, b, of, s, len, nullptr, &p);
    };
    CHECK(rc(keys, 3, ik, pos, n, B, off, S, need) == CHIP_OK && p.work == 2 && p.keys_used == 1);
    CHECK(rc(nullptr, 3, ik, pos, n, B, off, S, need) == CHIP_ERR_INVALID_ARG);
    CHECK(rc(keys, uint64_t(1) << 31, ik, pos, n, B, off, S, need) == CHIP_ERR_INVALID_ARG);
    const uint32_t bad_key[3] = {0, 2, 0};
    CHECK(rc(keys, 3, bad_key, pos, n, B, off, S, need) == CHIP_ERR_INVALID_ARG);
    const uint64_t far[3] = {5, 0, MAX_END - 16};
    CHECK(rc(keys, 3, ik, far, n, B, off, S, need) == CHIP_ERR_INVALID_ARG);
    const uint64_t wrap_pos[3] = {5, 0, ~uint64_t(0) - 3};
    CHECK(rc(keys, 3, ik, wrap_pos, n, B, off, S, need) == CHIP_ERR_INVALID_ARG);
    const uint64_t big_off[3] = {0, 8, (uint64_t(1) << 53) + 16};
    CHECK(rc(keys, 3, ik, pos, n, B, big_off, S, need) == CHIP_ERR_INVALID_ARG);
    CHECK(rc(keys, 3, ik, pos, n, 0, off, S, need) == CHIP_ERR_INVALID_ARG);
    const uint64_t odd_off[3] = {0, 8, 120};
    CHECK(rc(keys, 3, ik, pos, n, B, odd_off, S, need) == CHIP_ERR_INVALID_ARG);
    CHECK(rc(keys, 3, ik, pos, n, B, off, S + 8, need) == CHIP_ERR_INVALID_ARG);
    const uint64_t over[3] = {0, 8, 96};
    CHECK(rc(keys, 3, ik, pos, n, B, over, S, need) == CHIP_ERR_INVALID_ARG);
    CHECK(rc(keys, 3, ik, pos, n, B, off, S, need - 1) == CHIP_ERR_INVALID_ARG);
    const uint64_t none[3] = {0, 0, 0};
    CHECK(rc(keys, 3, ik, pos, none, 0, odd_off, S, need) == CHIP_OK && p.work == 0 && p.keys_used == 0);
    CHECK(scratch_len(2, 4) > need && scratch_len(3, 3) > need && scratch_len(0, 0) == 0);
    CHECK(spans_of(0) == 0 && spans_of(1) == 1 && spans_of(16 * SPAN_UNITS) == 1 && spans_of(16 * SPAN_UNITS + 1) == 2);
    const std::vector<uint64_t> sh = shifted(pos, 3);
    CHECK(sh[0] == 102 && sh[1] == 97 && sh[2] == 196);
}

int main() {
    std::mt19937_64 rng(0xC0FFEE);
    check_ks_shift();
    check_j0(rng);
    check_edges(rng);
    check_wrap(rng);
    check_plan();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
