// snap_device_check.cpp — the text the snappy kernels compile
// (carbonado_amd/csrc/snap_device.hpp) and the host plan (snap_plan.hpp), run
// on the host against host_snap.cpp.  Stand-alone: built with ASan + UBSan by
// tests/test_snap_dev_cpu.py together with host_snap.cpp and run directly.
//
//   * CRC: the 64 lane terms (table CRC of a segment, moved over the bytes
//     behind it by square-and-multiply) XORed and finished, against
//     host::crc_masked at every length 0..130 and at 65535 / 65536.
//   * compress: every object walked as the kernels split it (one block at a
//     time into a private slot of SLOT_PITCH bytes, the raw rule and the chunk
//     offsets per object, then header and body at their byte offsets), against
//     host::snap_compress byte for byte.
//   * decode: decode_block on every compressed block and on corrupted copies
//     of it (flipped bytes, cuts, forged tags) against host::decompress_raw:
//     same verdict, same bytes; the stage buffer is exactly the block's
//     length, so a write past it is an ASan report.
//   * the plan: tables and refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/host_stages.hpp"
#include "../carbonado_amd/csrc/snap_internal.hpp"
#include "../carbonado_amd/csrc/snap_plan.hpp"

using namespace chip;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static uint32_t crc_by_lanes(const uint8_t *p, size_t n) {
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = snap::crc_table_entry(i);
    uint32_t x = 0;
    for (uint32_t lane = 0; lane < snap::LANES; ++lane) x ^= snap::crc_lane_term(tab, p, n, lane);
    return snap::crc_finish(x, n);
}

// random runs of 1..L bytes alternating with repeats of earlier output
static std::vector<uint8_t> mix(size_t n, unsigned L, uint32_t seed) {
    static const unsigned reps[] = {4, 5, 7, 11, 12, 20, 59, 60, 61, 64, 65, 67, 68, 69, 130, 300};
    std::mt19937 g(seed);
    std::vector<uint8_t> v;
    v.reserve(n + 400);
    while (v.size() < n) {
        const unsigned run = 1 + g() % L;
        for (unsigned i = 0; i < run; ++i) v.push_back(uint8_t(g()));
        const unsigned len = reps[g() % 16];
        size_t off;
        switch (g() % 3) {
            case 0: off = 1 + g() % 8; break;
            case 1: off = 9 + g() % 2039; break;
            default: off = 2048 + g() % 63488; break;
        }
        if (off > v.size()) off = v.size();
        for (unsigned i = 0; i < len && off; ++i) v.push_back(v[v.size() - off]);
    }
    v.resize(n);
    return v;
}

struct Block {
    std::vector<uint8_t> body;  // compress_block's output
    size_t ulen;
};
static std::vector<Block> g_blocks;

// the three kernels' work for one object, on the host
static std::vector<uint8_t> snap_as_kernels(const std::vector<uint8_t> &in) {
    const uint64_t n = in.size(), nb = snap::blocks_of(n);
    std::vector<std::unique_ptr<uint8_t[]>> slots;
    std::vector<snap::CMeta> meta(nb);
    auto table = std::make_unique<uint16_t[]>(snap::TABLE_MAX);
    snap::OneThread w;
    for (uint64_t k = 0; k < nb; ++k) {  // block kernel
        const size_t len = size_t(std::min<uint64_t>(snap::MAX_BLOCK, n - k * snap::MAX_BLOCK));
        slots.emplace_back(new uint8_t[snap::SLOT_PITCH]);
        const uint8_t *src = in.data() + k * snap::MAX_BLOCK;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);  // reads past the block are reports
        std::memcpy(exact.get(), src, len);
        meta[k].clen = uint32_t(snap::compress_block(w, slots[k].get(), exact.get(), len, table.get()));
        meta[k].crc = crc_by_lanes(exact.get(), len);
        CHECK(meta[k].clen <= snap::MAX_COMPRESS_BLOCK, "slot overflow %u", meta[k].clen);
        g_blocks.push_back({std::vector<uint8_t>(slots[k].get(), slots[k].get() + meta[k].clen), len});
    }
    uint64_t pos = n ? 10 : 0;  // frame kernel
    for (uint64_t k = 0; k < nb; ++k) {
        const uint64_t len = std::min<uint64_t>(snap::MAX_BLOCK, n - k * snap::MAX_BLOCK);
        const bool raw = meta[k].clen >= len - len / 8;
        meta[k].off = pos | (raw ? snap::CMETA_RAW : 0);
        pos += 8 + (raw ? len : meta[k].clen);
    }
    std::vector<uint8_t> out(pos);
    if (n) std::memcpy(out.data(), host::STREAM_ID, 10);
    for (uint64_t k = 0; k < nb; ++k) {  // gather kernel
        const uint64_t len = std::min<uint64_t>(snap::MAX_BLOCK, n - k * snap::MAX_BLOCK);
        const bool raw = meta[k].off & snap::CMETA_RAW;
        const uint64_t blen = raw ? len : meta[k].clen;
        uint8_t *chunk = out.data() + (meta[k].off & ~snap::CMETA_RAW);
        const uint32_t cl = uint32_t(4 + blen);
        chunk[0] = raw ? 1 : 0;
        chunk[1] = uint8_t(cl);
        chunk[2] = uint8_t(cl >> 8);
        chunk[3] = uint8_t(cl >> 16);
        std::memcpy(chunk + 4, &meta[k].crc, 4);
        std::memcpy(chunk + 8, raw ? in.data() + k * snap::MAX_BLOCK : slots[k].get(), blen);
    }
    return out;
}

static void check_compress(const std::vector<uint8_t> &in, const char *what) {
    std::vector<uint8_t> want(host::snap_max_len(in.size()) + 1);
    uint64_t wl = 0;
    CHECK(host::snap_compress(in.data(), in.size(), want.data(), want.size(), &wl) == CHIP_OK, "host %s", what);
    want.resize(wl);
    const std::vector<uint8_t> got = snap_as_kernels(in);
    CHECK(got == want, "%s n=%zu: %zu bytes against the host's %zu", what, in.size(), got.size(), want.size());
    CHECK(snap::max_len(in.size()) == host::snap_max_len(in.size()), "max_len %zu", in.size());
}

// both decoders on src[0, n) for a block of ulen bytes
static void check_decode(const uint8_t *src_, size_t n, size_t ulen, const char *what) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[n ? n : 1]);
    std::memcpy(src.get(), src_, n);
    std::unique_ptr<uint8_t[]> a(new uint8_t[ulen ? ulen : 1]), b(new uint8_t[ulen ? ulen : 1]);
    std::memset(a.get(), 0xEE, ulen);
    std::memset(b.get(), 0xEE, ulen);
    size_t la = 0, lb = 0;
    snap::OneThread w;
    const bool oka = snap::decode_block(w, src.get(), n, a.get(), ulen, &la) && la == ulen;
    const bool okb = host::decompress_raw(src.get(), n, b.get(), ulen, &lb) && lb == ulen;
    CHECK(oka == okb, "%s: verdict %d against the host's %d (n=%zu ulen=%zu)", what, oka, okb, n, ulen);
    if (oka && okb) CHECK(std::memcmp(a.get(), b.get(), ulen) == 0, "%s: bytes differ", what);
}

static void check_plan() {
    const uint64_t n[3] = {100000, 0, 17}, in_off[3] = {0, 100000, 100016}, out_off[3] = {3, 200000, 200001};
    snap::CPlan p;
    const uint64_t need = snap::snap_scratch_len(n, 3);
    CHECK(need && need % 16 == 0, "scratch");
    CHECK(snap::plan_snap(0x1000, in_off, n, 3, 0x100000, out_off, true, 0x9000000, need, &p) == CHIP_OK, "plan");
    CHECK(p.blocks == 3 && p.lay.total == need, "blocks");
    const snap::CBlk *blks = reinterpret_cast<const snap::CBlk *>(p.table.data() + p.lay.blks);
    CHECK(blks[1].obj == 0 && blks[1].idx == 1 && blks[2].obj == 2 && blks[2].idx == 0, "block table");
    CHECK(snap::plan_snap(0x1000, in_off, n, 3, 0x100000, out_off, true, 0x9000000, need - 1, &p) == CHIP_ERR_INVALID_ARG,
          "short scratch");
    const uint64_t bad_off[3] = {8, 100000, 100016};
    CHECK(snap::plan_snap(0x1000, bad_off, n, 3, 0x100000, out_off, true, 0x9000000, need, &p) == CHIP_ERR_INVALID_ARG,
          "alignment");
    const uint64_t lap[3] = {3, 200000, 100000};
    CHECK(snap::plan_snap(0x1000, in_off, n, 3, 0x100000, lap, true, 0x9000000, need, &p) == CHIP_ERR_INVALID_ARG,
          "overlap");
    const uint64_t in_len[2] = {500, 0}, cap[2] = {65537, 0}, uoff[2] = {0, 65552};
    snap::UPlan u;
    const uint64_t un = snap::unsnap_scratch_len(in_len, cap, 2);
    CHECK(un && un % 16 == 0, "unsnap scratch");
    CHECK(snap::plan_unsnap(0x1001, uoff, in_len, 2, 0x100000, uoff, cap, true, true, 0x9000000, un, &u) == CHIP_OK, "uplan");
    CHECK(u.slots == 3 + 1, "slots %llu", (unsigned long long)u.slots);
    CHECK(snap::plan_unsnap(0x1001, uoff, in_len, 2, 0x100008, uoff, cap, true, true, 0x9000000, un, &u) ==
              CHIP_ERR_INVALID_ARG, "uplan alignment");
}

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? uint32_t(std::strtoul(argv[1], nullptr, 0)) : 1;
    const bool big = argc > 2 && !std::strcmp(argv[2], "big");
    std::mt19937 g(seed);

    // CRC
    {
        std::vector<uint8_t> buf(65536);
        for (auto &x : buf) x = uint8_t(g());
        for (size_t n = 0; n <= 130; ++n)
            CHECK(crc_by_lanes(buf.data() + (n & 7), n) == host::crc_masked(buf.data() + (n & 7), n), "crc n=%zu", n);
        for (size_t n : {size_t(65535), size_t(65536), size_t(4097), size_t(1000)})
            CHECK(crc_by_lanes(buf.data(), n) == host::crc_masked(buf.data(), n), "crc n=%zu", n);
    }

    // compress
    const size_t sizes[] = {0, 1, 16, 17, 18, 255, 256, 257, 512, 513, 4096, 4097, 16384, 16385, 65535, 65536, 65537,
                            131073, 200000};
    for (size_t n : sizes) {
        std::vector<uint8_t> r(n);
        for (auto &x : r) x = uint8_t(g());
        check_compress(r, "random");
        check_compress(std::vector<uint8_t>(n, 0), "zeros");
        check_compress(mix(n, 40, seed + uint32_t(n)), "mix40");
        if (n >= 4096) {
            check_compress(mix(n, 300, seed + 7 + uint32_t(n)), "mix300");
            check_compress(mix(n, 400, seed + 9 + uint32_t(n)), "mix400");
        }
        std::vector<uint8_t> text(n);
        for (size_t i = 0; i < n; ++i) text[i] = "the quick brown fox jumps over the lazy dog. "[(i * 7 + i / 13) % 45];
        check_compress(text, "text");
    }
    if (big) check_compress(mix((size_t(1) << 20) + 12345, 40, seed), "mix40 1 MiB");

    // decode: every block above, whole and damaged
    size_t tried = 0;
    for (const Block &b : g_blocks) {
        check_decode(b.body.data(), b.body.size(), b.ulen, "whole");
        const int rounds = b.body.size() > 20000 ? 3 : 12;
        for (int t = 0; t < rounds; ++t) {
            std::vector<uint8_t> c = b.body;
            switch (g() % 5) {
                case 0: c[g() % c.size()] ^= uint8_t(1u << (g() % 8)); break;
                case 1: c.resize(g() % c.size()); break;
                case 2: c[g() % c.size()] = uint8_t(g()); break;
                case 3: {  // a forged tag somewhere, of any kind
                    const size_t at = g() % c.size();
                    c[at] = uint8_t(g());
                    if (at + 4 < c.size() && (g() & 1)) c[at + 1] = c[at + 2] = c[at + 3] = c[at + 4] = 0;
                    break;
                }
                default: c.push_back(uint8_t(g())); break;
            }
            check_decode(c.data(), c.size(), b.ulen, "damaged");
            if (b.ulen) check_decode(c.data(), c.size(), b.ulen - 1, "short capacity");
            ++tried;
        }
    }
    // hand-built bodies: copy-4, 4- and 5-byte literal headers, overlapping copies, the refusals
    {
        std::vector<uint8_t> v = {20, 0xF0, 3, 'a', 'b', 'c', 'd'};  // literal with a 1-byte length
        v.insert(v.end(), {uint8_t((3 << 2) | 3), 4, 0, 0, 0});      // copy-4: len 4 off 4
        v.insert(v.end(), {uint8_t((11 << 2) | 2), 1, 0});           // copy-2: len 12 off 1
        check_decode(v.data(), v.size(), 20, "copy-4");
        for (uint8_t off = 1; off <= 7; ++off) {
            std::vector<uint8_t> o = {71, uint8_t(6 << 2), 1, 2, 3, 4, 5, 6, 7, uint8_t((63 << 2) | 2), off, 0};
            check_decode(o.data(), o.size(), 71, "overlap");
        }
        std::vector<uint8_t> l4 = {5, uint8_t(62 << 2), 4, 0, 0, 'h', 'e', 'l', 'l', 'o'};
        check_decode(l4.data(), l4.size(), 5, "4-byte literal header");
        std::vector<uint8_t> l5 = {5, uint8_t(63 << 2), 4, 0, 0, 0, 'h', 'e', 'l', 'l', 'o'};
        check_decode(l5.data(), l5.size(), 5, "5-byte literal header");
        std::vector<uint8_t> z0 = {8, uint8_t(3 << 2), 1, 2, 3, 4, uint8_t((3 << 2) | 2), 0, 0};
        check_decode(z0.data(), z0.size(), 8, "offset 0");
        std::vector<uint8_t> far = {8, uint8_t(3 << 2), 1, 2, 3, 4, uint8_t((3 << 2) | 2), 5, 0};
        check_decode(far.data(), far.size(), 8, "offset past written");
        std::vector<uint8_t> lit = {8, uint8_t(7 << 2), 1, 2, 3, 4};
        check_decode(lit.data(), lit.size(), 8, "literal past the body");
        std::vector<uint8_t> over = {6, uint8_t(3 << 2), 1, 2, 3, 4, uint8_t((3 << 2) | 2), 4, 0};
        check_decode(over.data(), over.size(), 6, "copy past the block");
        std::vector<uint8_t> big_len = {0x81, 0x80, 0x04, 0};
        check_decode(big_len.data(), big_len.size(), 65536, "varint 65537");
        std::vector<uint8_t> shrt = {9, uint8_t(3 << 2), 1, 2, 3, 4};
        check_decode(shrt.data(), shrt.size(), 9, "short of its varint");
        check_decode(shrt.data(), 0, 0, "empty body");
        const uint8_t zero[1] = {0};
        check_decode(zero, 1, 0, "zero-length block");
    }
    check_plan();
    std::printf("snap_device_check seed=%u: %zu blocks, %zu damaged bodies, %d failures\n", seed, g_blocks.size(), tried,
                failures);
    return failures ? 1 : 0;
}
