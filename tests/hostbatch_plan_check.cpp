// hostbatch_plan_check.cpp — the planning arithmetic of encode() / decode() from
// host memory (carbonado_amd/csrc/hostbatch_plan.hpp) driven stand-alone, for a
// build with -fsanitize=address,undefined (tests/test_hostbatch_cpu.py).  No
// device.
//
//  * the host-made region of a stream (HostGeo) against a brute-force pre-order
//    walk of the bao stream written here: the chunk slots and node runs tile
//    [8, t0) exactly, the compact offsets are ascending and dense, nbytes is
//    the runs' bytes, the tail's slots and runs tile [t0, bao_len); "t0 N x"
//    is printed per (N, N / 2) for the pytest to compare with bench.py's own
//    statement of it;
//  * slice sizing as a literal table, derived by hand from the expressions the
//    two host batches had inline;
//  * encode's bounds at levels 4, 8, 12..15: the formulas restated, and
//    final_max >= the final length of every host-stage output length up to
//    h_max that passes the slice-count check;
//  * dec_geom: statuses and lengths of damaged and intact headers.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../carbonado_amd/csrc/hostbatch_plan.hpp"

using namespace chip;
using hostbatch::HostGeo;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

// ---- the region geometry ----------------------------------------------------------------
struct Piece {
    uint64_t off, len;
    bool chunk;
    uint64_t index;  // of the chunk
};

// bao's pre-order: a subtree of cnt > 1 chunks is its parent node (64 B), its left
// subtree (the largest power of two below cnt) and its right subtree
static void walk(uint64_t s, uint64_t cnt, uint64_t zl, uint64_t *pos, std::vector<Piece> *out) {
    if (cnt == 1) {
        const uint64_t len = zl - 1024 * s < 1024 ? zl - 1024 * s : 1024;
        out->push_back({*pos, len, true, s});
        *pos += len;
        return;
    }
    out->push_back({*pos, 64, false, 0});
    *pos += 64;
    uint64_t left = 1;
    while (2 * left < cnt) left *= 2;
    walk(s, left, zl, pos, out);
    walk(s + left, cnt - left, zl, pos, out);
}

// the pieces tile [from, to) in ascending order, no gap and no overlap
static bool tiles(std::vector<std::pair<uint64_t, uint64_t>> iv, uint64_t from, uint64_t to) {
    std::sort(iv.begin(), iv.end());
    uint64_t pos = from;
    for (const auto &p : iv) {
        if (p.first != pos) return false;
        pos += p.second;
    }
    return pos == to;
}

static void check_geo(uint64_t zl, uint64_t nh, bool tail) {
    const uint64_t N = zl == 0 ? 1 : (zl + 1023) / 1024;
    std::vector<Piece> w;
    uint64_t end = 8;
    walk(0, N, zl, &end, &w);
    EXPECT(end == 8 + zl + 64 * (N - 1));
    std::vector<uint64_t> coff(N), clen(N);
    for (const Piece &p : w)
        if (p.chunk) coff[p.index] = p.off, clen[p.index] = p.len;
    const uint64_t t0 = nh ? coff[nh - 1] + clen[nh - 1] : 8;
    uint64_t nodes_before = 0;
    for (const Piece &p : w) nodes_before += !p.chunk && p.off < t0;

    const HostGeo g = hostbatch::host_geo(zl, nh, tail);
    EXPECT(g.N == N && g.nh == nh && g.zl == zl && g.t0 == t0);
    EXPECT(g.coff.size() == (tail ? N : nh));
    for (uint64_t i = 0; i < g.coff.size(); ++i) EXPECT(g.coff[i] == coff[i]);
    // the head: chunk slots and runs tile [8, t0); compact offsets ascending and dense
    std::vector<std::pair<uint64_t, uint64_t>> iv;
    for (uint64_t i = 0; i < nh; ++i) iv.push_back({g.coff[i], clen[i]});
    uint64_t src = 0;
    for (const HostGeo::Run &r : g.runs) {
        EXPECT(r.src == src && r.len > 0 && r.len % 64 == 0);
        src += r.len;
        iv.push_back({r.dst, r.len});
    }
    EXPECT(tiles(iv, 8, t0));
    EXPECT(g.nbytes == src && g.nbytes == 64 * nodes_before);
    // the tail: its slots and runs tile [t0, end)
    if (!tail) {
        EXPECT(g.truns.empty());
        return;
    }
    iv.clear();
    for (uint64_t i = nh; i < N; ++i) iv.push_back({g.coff[i], clen[i]});
    for (const HostGeo::Run &r : g.truns) {
        EXPECT(r.len > 0 && r.len % 64 == 0);
        iv.push_back({r.dst, r.len});
    }
    EXPECT(tiles(iv, t0, end));
}

static void check_geometry() {
    const uint64_t Ns[] = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 16384};
    for (uint64_t N : Ns) {
        for (uint64_t nh : {uint64_t(1), N / 2, N}) {
            if (nh < 1) continue;
            check_geo(1024 * N, nh, true);
            check_geo(1024 * N, nh, false);
        }
        check_geo(1024 * (N - 1) + 1, N, true);  // a short last chunk the host holds
        check_geo(1024 * (N - 1) + 1023, N, true);
        if (N < 2) continue;
        const HostGeo g = hostbatch::host_geo(1024 * N, N / 2);
        std::printf("t0 %llu %llu\n", (unsigned long long)N, (unsigned long long)g.t0);
    }
}

// ---- slice sizing ---------------------------------------------------------------------------
static void check_slices() {
    struct Row {
        uint32_t nslots;
        uint64_t slice_bytes;
        uint32_t host_threads, hw;
        uint64_t max_bytes, count;
        bool round;
        uint32_t want_nslots, want_T;
        uint64_t want_S, want_nslices;
    };
    const uint64_t MiB = 1ull << 20;
    const Row rows[] = {
        // the defaults at the benchmark's shape: 3 slots, 256 MiB slices of 16 MiB objects
        {0, 0, 0, 16, 16 * MiB, 1024, true, 3, 16, 16, 64},
        {3, 256 * MiB, 16, 200, 16 * MiB, 1024, true, 3, 16, 16, 64},
        // nslots clamped to 1..8
        {1, 0, 0, 16, 16 * MiB, 1024, true, 1, 16, 16, 64},
        {8, 0, 0, 16, 16 * MiB, 1024, true, 8, 16, 16, 64},
        {9, 0, 0, 16, 16 * MiB, 1024, true, 8, 16, 16, 64},
        // a slice smaller than one object: one object per slice (1 < (3 + 1) / 2: not rounded)
        {2, 1000, 3, 16, 10000, 5, true, 2, 3, 1, 5},
        // objects of 0 bytes: the divisor is 1, S = 256 MiB, then the count
        {3, 0, 4, 16, 0, 7, true, 3, 4, 7, 1},
        // host_threads 0: the hardware's, at least 1, at most 64; 100 asked for: 64
        {3, 1000, 0, 0, 100, 25, true, 3, 1, 10, 3},
        {3, 1000, 0, 1, 100, 25, true, 3, 1, 10, 3},
        {3, 1000, 0, 16, 100, 25, true, 3, 16, 16, 2},   // 10 >= 8: up to 16
        {3, 1000, 0, 200, 100, 25, true, 3, 64, 10, 3},  // 10 < 32: as it is
        {3, 1000, 100, 16, 100, 25, true, 3, 64, 10, 3},
        // the rounding threshold (T + 1) / 2, T odd and even
        {3, 300, 7, 16, 100, 100, true, 3, 7, 3, 34},
        {3, 400, 7, 16, 100, 100, true, 3, 7, 7, 15},
        {3, 300, 8, 16, 100, 100, true, 3, 8, 3, 34},
        {3, 400, 8, 16, 100, 100, true, 3, 8, 8, 13},
        // fewer objects than a slice holds
        {3, 400, 7, 16, 100, 5, true, 3, 7, 5, 1},
        {3, 0, 16, 16, 16 * MiB, 3, true, 3, 16, 3, 1},
        // decode's form, and encode's without host work per object: no rounding
        {3, 400, 7, 16, 100, 100, false, 3, 7, 4, 25},
        {2, 20000, 3, 16, 10000, 5, false, 2, 3, 2, 3},
        {0, 0, 0, 200, 16 * MiB, 1024, false, 3, 64, 16, 64},
        {3, 1000, 3, 16, 10000, 5, false, 3, 3, 1, 5},
    };
    for (const Row &r : rows) {
        const hostbatch::Slices p =
            hostbatch::plan_slices(r.nslots, r.slice_bytes, r.host_threads, r.hw, r.max_bytes, r.count, r.round);
        const bool ok = p.nslots == r.want_nslots && p.T == r.want_T && p.S == r.want_S && p.nslices == r.want_nslices;
        if (!ok)
            std::printf("row %d: got {%u, %u, %llu, %llu}\n", (int)(&r - rows), p.nslots, p.T, (unsigned long long)p.S,
                        (unsigned long long)p.nslices);
        EXPECT(ok);
    }
}

// ---- encode's bounds ------------------------------------------------------------------------
static void check_bounds() {
    for (uint8_t level : {4, 8, 12, 13, 14, 15})
        for (uint64_t n : {0ull, 1ull, 4096ull, 70001ull}) {
            const bool ecies = level & 1, snappy = level & 2, bao = level & 4, zfec = level & 8;
            // restated: the snappy frame's bound (a 10-B identifier, 8 B per 64 KiB block), the
            // envelope's 97 B, zfec's padding to 4 KiB and its doubling, bao's header and parents
            uint64_t h = n;
            if (snappy && n) h = 10 + 8 * ((n + 65535) / 65536) + n;
            if (ecies) h += 97;
            const uint64_t z = zfec ? 2 * ((h + 4095) / 4096 * 4096) : h;
            const uint64_t f = bao ? 8 + z + 64 * ((z ? (z + 1023) / 1024 : 1) - 1) : z;
            const hostbatch::EncodeBounds b = hostbatch::encode_bounds(level, n);
            EXPECT(b.h_max == h && b.zlen_max == z && b.final_max == f);
            EXPECT(hostbatch::host_stage_max(level, n) == h);
            if (zfec) EXPECT(hostbatch::split_chunks(h) == z / 1024);
            chip_encode_info inf;
            uint64_t zl = 0, fl = 0;
            const int st = hostbatch::encode_info_for(level, n, h, 0, 0, &inf, &zl, &fl);
            EXPECT(b.st == (hostbatch::has_host_stages(level) ? CHIP_OK : st));
            if (st == CHIP_OK) {
                EXPECT(zl == z && fl == f && inf.output_len == (uint32_t)f && inf.input_len == (uint32_t)n);
                EXPECT(inf.chunk_len == (zfec ? z / 8 : 0) && inf.padding_len == (zfec ? z / 2 - h : 0));
                EXPECT(inf.bytes_verifiable == (bao ? (uint32_t)f : 0));
            }
            // every output length the host stages may leave
            uint64_t passed = 0;
            for (uint64_t len = 0; len <= h; ++len) {
                if (hostbatch::encode_info_for(level, n, len, 0, 0, &inf, &zl, &fl) != CHIP_OK) continue;
                ++passed;
                if (fl > b.final_max || zl > b.zlen_max) {
                    EXPECT(fl <= b.final_max && zl <= b.zlen_max);
                    break;
                }
            }
            EXPECT(passed > 0);
        }
}

// ---- decode's geometry ----------------------------------------------------------------------
static std::vector<uint8_t> header(uint64_t v) {
    std::vector<uint8_t> h(8);
    for (int i = 0; i < 8; ++i) h[i] = (uint8_t)(v >> (8 * i));
    return h;  // dec_geom reads the header alone: a byte past it is a sanitizer report
}

static void check_dec_geom() {
    using hostbatch::dec_geom;
    const uint8_t BAO = CHIP_FORMAT_BAO, ZFEC = CHIP_FORMAT_ZFEC;
    // an object of 10 000 bytes: padded to 12 288, 8 shards of 3072, a stream of 24 chunks
    const uint64_t zl = 24576, slen = rules::bao_len(zl);
    const uint32_t pad = 2288;
    EXPECT(slen == 8 + 24576 + 64 * 23);
    std::vector<uint8_t> h = header(zl);
    hostbatch::DecGeom g = dec_geom(BAO | ZFEC, h.data(), slen, pad);  // intact at level 12
    EXPECT(g.st == CHIP_OK && g.blen == zl && g.olen == 10000);
    g = dec_geom(ZFEC, nullptr, zl, pad);  // ... at level 8: no header read
    EXPECT(g.st == CHIP_OK && g.blen == zl && g.olen == 10000);
    h = header(10000);
    g = dec_geom(BAO, h.data(), rules::bao_len(10000), 77);  // ... at level 4: the padding is zfec's alone
    EXPECT(g.st == CHIP_OK && g.blen == 10000 && g.olen == 10000);
    // the header three bytes short of its stream
    h = header(zl);
    g = dec_geom(BAO | ZFEC, h.data(), slen - 3, pad);
    EXPECT(g.st == CHIP_ERR_BAO_TRUNCATED && g.st != CHIP_OK);
    std::printf("header_short_status %d\n", g.st);
    // a length field larger than the stream, by one and by far; no room for a header
    h = header(slen + 1);
    EXPECT(dec_geom(BAO | ZFEC, h.data(), slen, pad).st == CHIP_ERR_BAO_TRUNCATED);
    h = header(~0ull);
    EXPECT(dec_geom(BAO, h.data(), slen, 0).st == CHIP_ERR_BAO_TRUNCATED);
    EXPECT(dec_geom(BAO, nullptr, 7, 0).st == CHIP_ERR_BAO_TRUNCATED);
    // a longer buffer than the stream is fine
    h = header(zl);
    EXPECT(dec_geom(BAO | ZFEC, h.data(), slen + 5, pad).st == CHIP_OK);
    // an uneven zfec length, with and without bao
    g = dec_geom(ZFEC, nullptr, 8 * 1024 + 1, 0);
    EXPECT(g.st == CHIP_ERR_UNEVEN_ZFEC_CHUNKS && g.blen == 8193 && g.olen == 8193);
    h = header(8193);
    EXPECT(dec_geom(BAO | ZFEC, h.data(), rules::bao_len(8193), 0).st == CHIP_ERR_UNEVEN_ZFEC_CHUNKS);
    // padding: 4 C is an empty object, one above is an error
    g = dec_geom(ZFEC, nullptr, 8192, 4096);
    EXPECT(g.st == CHIP_OK && g.olen == 0);
    g = dec_geom(ZFEC, nullptr, 8192, 4097);
    EXPECT(g.st == CHIP_ERR_ZFEC && g.olen == 8192);
    g = dec_geom(ZFEC, nullptr, 0, 0);
    EXPECT(g.st == CHIP_OK && g.olen == 0);
    EXPECT(dec_geom(ZFEC, nullptr, 0, 1).st == CHIP_ERR_ZFEC);
    // neither stage: the input as it is
    g = dec_geom(0, nullptr, 123, 9);
    EXPECT(g.st == CHIP_OK && g.blen == 123 && g.olen == 123);
}

int main() {
    check_geometry();
    check_slices();
    check_bounds();
    check_dec_geom();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
