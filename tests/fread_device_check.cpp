// fread_device_check.cpp — the text the frame-read kernels compile
// (carbonado_amd/csrc/fread_device.hpp) on one host thread, against
// host_snap.cpp.  Stand-alone: built with ASan + UBSan by
// tests/test_fread_cpu.py together with host_snap.cpp and run directly.
//
//   * the walk and the chain check over frame streams written by
//     host::snap_compress (sizes around one, two and four frames, compressible
//     and random), and over hand-built ones: a skippable chunk, a repeated
//     identifier, a short inner block, an empty block, an identifier alone, a
//     truncated last chunk, a bad length, a reserved type, a zero-length
//     object, capacity one too small.  The offsets array is exactly the
//     capacity, so a write past it is an ASan report.
//   * the chain check of wrong indexes: an entry off by one, two exchanged, a
//     frame dropped, a last entry that is not L, a header read that failed.
//   * a frame as the block kernel serves it (header against the index,
//     decode_block with the OneThread policy, CRC by lanes, lane_store of a
//     sub-range) against slices of host::snap_decompress's output at every
//     start and end residue mod 16, into a buffer of exactly the range.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/fread_device.hpp"
#include "../carbonado_amd/csrc/host_stages.hpp"
#include "../carbonado_amd/csrc/snap_internal.hpp"

using namespace chip;
using fread::ST_OK;
using fread::ST_SNAP;
using fread::ST_TOO_SMALL;
using fread::ST_UNSUPPORTED;

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

typedef std::vector<uint8_t> Bytes;

static Bytes random_bytes(size_t n, uint32_t seed) {
    std::mt19937 g(seed);
    Bytes v(n);
    for (auto &b : v) b = uint8_t(g());
    return v;
}

// random runs of 1..40 bytes alternating with repeats of earlier output
static Bytes mix(size_t n, uint32_t seed) {
    std::mt19937 g(seed);
    Bytes v;
    while (v.size() < n) {
        const unsigned run = 1 + g() % 40;
        for (unsigned i = 0; i < run; ++i) v.push_back(uint8_t(g()));
        size_t off = 1 + g() % 3000;
        if (off > v.size()) off = v.size();
        const unsigned len = 4 + g() % 100;
        for (unsigned i = 0; i < len && off; ++i) v.push_back(v[v.size() - off]);
    }
    v.resize(n);
    return v;
}

static Bytes compress(const Bytes &in) {
    Bytes out(host::snap_max_len(in.size()) + 1);
    uint64_t n = 0;
    if (host::snap_compress(in.data(), in.size(), out.data(), out.size(), &n) != 0) std::abort();
    out.resize(n);
    return out;
}

static Bytes chunk(uint8_t ty, const Bytes &body) {
    Bytes c = {ty, uint8_t(body.size()), uint8_t(body.size() >> 8), uint8_t(body.size() >> 16)};
    c.insert(c.end(), body.begin(), body.end());
    return c;
}
static Bytes raw_chunk(const Bytes &content) {
    const uint32_t crc = host::crc_masked(content.data(), content.size());
    Bytes body = {uint8_t(crc), uint8_t(crc >> 8), uint8_t(crc >> 16), uint8_t(crc >> 24)};
    body.insert(body.end(), content.begin(), content.end());
    return chunk(0x01, body);
}
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes v;
    for (const Bytes &p : parts) v.insert(v.end(), p.begin(), p.end());
    return v;
}
static const Bytes IDENT(host::STREAM_ID, host::STREAM_ID + 10);

// frame-stream bytes straight from a vector, exactly n of them: more is an ASan report
struct Fetch {
    const Bytes *f;
    void operator()(uint64_t pos, uint32_t n, uint8_t *b) {
        Bytes exact(f->begin() + pos, f->begin() + pos + n);
        std::memset(b, 0xEE, fread::HDR_READ);
        std::memcpy(b, exact.data(), n);
    }
};

struct Walked {
    fread::WalkOut out;
    std::vector<uint64_t> off;
};
static Walked walk(const Bytes &frame, uint32_t cap) {
    Walked w;
    w.off.assign(cap, ~uint64_t(0));
    Fetch f{&frame};
    w.out = fread::walk(f, frame.size(), w.off.data(), cap);
    return w;
}

// the reference walk: every chunk's offset, whatever it is
static std::vector<uint64_t> chunks_of(const Bytes &frame) {
    std::vector<uint64_t> off;
    uint64_t pos = frame.empty() ? 0 : 10;
    while (pos < frame.size()) {
        off.push_back(pos);
        pos += 4 + (uint64_t(frame[pos + 1]) | uint64_t(frame[pos + 2]) << 8 | uint64_t(frame[pos + 3]) << 16);
    }
    off.push_back(frame.size());
    return off;
}

// the chain kernel's work for one stream on one thread: rows staged as the header reads stage them
static uint32_t chain(const Bytes &frame, const std::vector<uint64_t> &off, uint64_t *plain, uint32_t fail_read = ~0u,
                      uint32_t fail_status = 0) {
    const uint32_t nframes = uint32_t(off.size() - 1);
    fread::VStream v{};
    v.L = frame.size();
    v.nframes = nframes;
    Bytes rows(size_t(fread::ROW) * off.size(), 0xEE);
    std::vector<uint32_t> rstat(off.size(), 0), rvouch(off.size(), 0);
    for (uint32_t e = 0; e < off.size(); ++e) {
        const uint64_t at = e == 0 ? 0 : off[e - 1], want = e == 0 ? fread::ID_LEN : fread::HDR_READ;
        if (at >= v.L) continue;
        const uint64_t n = v.L - at < want ? v.L - at : want;
        std::memcpy(rows.data() + fread::ROW * e, frame.data() + at, n);
    }
    if (fail_read != ~0u) {
        rstat[fail_read] = fail_status;
        std::memset(rows.data() + fread::ROW * fail_read, 0, fread::ROW);
    }
    uint32_t bits = 0, vouch = 0, last = 0;
    for (uint32_t lane = 0; lane < fread::LANES; ++lane) {
        uint32_t mine = 0;
        bits |= fread::chain_lane(v, off.data(), rows.data(), rstat.data(), rvouch.data(), lane, fread::LANES, &vouch,
                                  &mine);
        last |= mine;
    }
    const uint32_t st = fread::chain_status(bits & 1, bits & 2, bits & 4, bits & 8);
    *plain = st == ST_OK && nframes ? uint64_t(fread::FRAME) * (nframes - 1) + last : 0;
    return st;
}

static void check_walk_and_chain() {
    const size_t sizes[] = {0, 1, 100, 65535, 65536, 65537, 131072, 131077, 200003, 262144};
    uint32_t seed = 1;
    for (size_t n : sizes)
        for (int kind = 0; kind < 2; ++kind) {
            const Bytes plain = kind ? mix(n, ++seed) : random_bytes(n, ++seed);
            const Bytes frame = compress(plain);
            const std::vector<uint64_t> want = chunks_of(frame);
            const uint32_t need = uint32_t(want.size());
            Walked w = walk(frame, need);
            CHECK(w.out.status == ST_OK && w.out.nframes == need - 1 && w.out.plain == n, "walk n=%zu kind=%d: %u", n, kind,
                  w.out.status);
            CHECK(w.off == want, "offsets n=%zu", n);
            w = walk(frame, need + 3);  // room to spare: the entries behind the index stay untouched
            CHECK(w.out.status == ST_OK && std::vector<uint64_t>(w.off.begin(), w.off.begin() + need) == want &&
                      w.off[need] == ~uint64_t(0), "spare n=%zu", n);
            w = walk(frame, need - 1);  // capacity one too small: it keeps counting
            CHECK(w.out.status == ST_TOO_SMALL && w.out.nframes == need - 1, "small n=%zu: %u", n, w.out.status);
            CHECK(std::vector<uint64_t>(want.begin(), want.begin() + need - 1) == w.off, "small offsets n=%zu", n);
            uint64_t pl = 0;
            CHECK(chain(frame, want, &pl) == ST_OK && pl == n, "chain n=%zu", n);
            if (need >= 3) {
                std::vector<uint64_t> bad = want;
                bad[1] += 1;
                CHECK(chain(frame, bad, &pl) == ST_SNAP && pl == 0, "off by one n=%zu", n);
                bad = want;
                std::swap(bad[0], bad[1]);
                CHECK(chain(frame, bad, &pl) == ST_SNAP, "exchanged n=%zu", n);
                bad = want;
                bad.erase(bad.begin() + 1);
                CHECK(chain(frame, bad, &pl) == ST_SNAP, "dropped n=%zu", n);
                CHECK(chain(frame, want, &pl, 2, 7) == 7 && pl == 0, "failed read n=%zu", n);
                CHECK(chain(frame, want, &pl, 1, 5) == 5, "contradicted read n=%zu", n);
            }
            if (need >= 2) {
                std::vector<uint64_t> bad = want;
                bad.back() -= 1;
                CHECK(chain(frame, bad, &pl) == ST_SNAP, "last entry n=%zu", n);
                bad = want;
                bad[0] = 9;
                CHECK(chain(frame, bad, &pl) == ST_SNAP, "first entry n=%zu", n);
                CHECK(chain(frame, want, &pl, 0, 7) == 7, "identifier read n=%zu", n);
            }
        }
    // hand-built streams
    const Bytes a = random_bytes(600, 50), full = random_bytes(65536, 51);
    struct Case {
        const char *name;
        Bytes frame;
        uint32_t want;
    };
    Bytes truncated = cat({IDENT, raw_chunk(full), raw_chunk(a)});
    truncated.resize(truncated.size() - 5);
    Bytes badlen = cat({IDENT, raw_chunk(full), raw_chunk(a)});
    badlen[10 + 1] ^= 0x40;  // the first chunk's length: the next header lies inside its bytes
    Bytes toolong = cat({IDENT, raw_chunk(a)});
    toolong[10 + 3] = 0x7F;
    Bytes big = cat({IDENT, raw_chunk(random_bytes(65537, 52))});
    Bytes varint = cat({IDENT, chunk(0x00, {1, 2, 3, 4, 0x80, 0x80, 0x80, 0x01, 0})});
    const Case cases[] = {
        {"skippable", cat({IDENT, chunk(0x80, {1, 2, 3}), raw_chunk(a)}), ST_UNSUPPORTED},
        {"padding", cat({IDENT, raw_chunk(full), chunk(0xFE, {}), raw_chunk(a)}), ST_UNSUPPORTED},
        {"repeated identifier", cat({IDENT, raw_chunk(full), IDENT, raw_chunk(a)}), ST_UNSUPPORTED},
        {"short inner block", cat({IDENT, raw_chunk(a), raw_chunk(full)}), ST_UNSUPPORTED},
        {"empty block", cat({IDENT, raw_chunk({})}), ST_UNSUPPORTED},
        {"identifier alone", IDENT, ST_UNSUPPORTED},
        {"truncated last chunk", truncated, ST_SNAP},
        {"bad length", badlen, ST_SNAP},
        {"length past the end", toolong, ST_SNAP},
        {"reserved type", cat({IDENT, chunk(0x02, {1, 2, 3, 4, 5})}), ST_SNAP},
        {"no crc", cat({IDENT, chunk(0x01, {1, 2, 3})}), ST_SNAP},
        {"block above 64 KiB", big, ST_SNAP},
        {"long varint", varint, ST_SNAP},
        {"no identifier", raw_chunk(a), ST_SNAP},
        {"short", Bytes(IDENT.begin(), IDENT.begin() + 7), ST_SNAP},
        {"canonical", cat({IDENT, raw_chunk(full), raw_chunk(a)}), ST_OK},
    };
    for (const Case &c : cases) {
        const Walked w = walk(c.frame, 8);
        CHECK(w.out.status == c.want, "%s: walk %u", c.name, w.out.status);
        if (c.want != ST_OK && w.out.nframes < 8)
            CHECK(w.off[w.out.nframes] == w.out.bad_pos, "%s: the position it stopped at", c.name);
        // the chain check of every chunk the stream has, where its headers chain at all
        if (c.want == ST_UNSUPPORTED || c.want == ST_OK) {
            uint64_t pl = 0;
            const uint32_t st = chain(c.frame, chunks_of(c.frame), &pl);
            CHECK(st == c.want && pl == (c.want == ST_OK ? 65536u + 600u : 0u), "%s: chain %u", c.name, st);
        }
    }
    uint64_t pl = 1;
    CHECK(chain(Bytes(), {0}, &pl) == ST_OK && pl == 0, "empty stream");
    CHECK(chain(Bytes(), {0, 0}, &pl) == ST_SNAP, "a frame in an empty stream");
    CHECK(chain(Bytes(), {5}, &pl) == ST_SNAP, "empty stream, wrong entry");
    CHECK(chain(cases[15].frame, {uint64_t(cases[15].frame.size())}, &pl) == ST_SNAP, "no frame in a stream with bytes");
}

// one (request, frame) as fread_block_kernel serves it; false: the frame is bad
static bool serve(const Bytes &row, const fread::Seg &sg, uint8_t *content) {
    if (sg.clen < 4) return false;
    const uint8_t *h = row.data() + sg.src;
    const uint32_t ty = h[0], clen = uint32_t(h[1]) | uint32_t(h[2]) << 8 | uint32_t(h[3]) << 16;
    const uint32_t want = snap::load32(h + 4);
    if (ty > 1 || clen != sg.clen) return false;
    const uint32_t dl = sg.clen - 4;
    Bytes stage(sg.ulen);  // exactly the block: a write past it is an ASan report
    const uint8_t *from = stage.data();
    if (ty == 1) {
        if (dl != sg.ulen) return false;
        from = h + 8;
    } else {
        snap::OneThread w;
        size_t got = 0;
        if (!snap::decode_block(w, h + 8, dl, stage.data(), sg.ulen, &got) || got != sg.ulen) return false;
    }
    uint32_t tab[256], x = 0;
    for (uint32_t i = 0; i < 256; ++i) tab[i] = snap::crc_table_entry(i);
    for (uint32_t lane = 0; lane < snap::LANES; ++lane) x ^= snap::crc_lane_term(tab, from, sg.ulen, lane);
    if (snap::crc_finish(x, sg.ulen) != want) return false;
    for (uint32_t lane = 0; lane < fread::LANES; ++lane) fread::lane_store(content + sg.dst, from + sg.lo, sg.hi - sg.lo, lane);
    return true;
}

static void check_store() {
    const Bytes plain = cat({mix(65536, 70), random_bytes(65536, 71), mix(3000, 72)});
    const Bytes frame = compress(plain);
    const std::vector<uint64_t> off = chunks_of(frame);
    CHECK(off.size() == 4 && frame[off[0]] == 0 && frame[off[1]] == 1, "a compressed and a raw frame");
    Bytes back(plain.size());
    uint64_t n = 0;
    CHECK(host::snap_decompress(frame.data(), frame.size(), back.data(), back.size(), &n) == 0 && back == plain, "decode");
    for (uint32_t f = 0; f < 3; ++f) {
        const uint32_t ulen = f == 2 ? 3000 : 65536;
        // the row starts at the frame's header, at a 16-B aligned address as the staging rows do
        Bytes row(frame.begin() + off[f], frame.begin() + off[f + 1]);
        for (uint32_t a = 0; a < 16; ++a)
            for (uint32_t e = 0; e < 16; ++e)
                for (uint32_t lo : {a, 1000 + a, ulen - 40 + a}) {
                    const uint32_t hi = lo + 17 + e + (lo == a ? 100 : 0) > ulen ? ulen : lo + 17 + e + (lo == a ? 100 : 0);
                    fread::Seg sg{};
                    sg.clen = uint32_t(off[f + 1] - off[f] - 4);
                    sg.ulen = ulen;
                    sg.lo = lo;
                    sg.hi = hi;
                    // the content range in a buffer of exactly its bytes
                    sg.dst = 0;
                    Bytes exact(hi - lo, 0xA5);
                    CHECK(serve(row, sg, exact.data()), "serve f=%u lo=%u hi=%u", f, lo, hi);
                    CHECK(std::memcmp(exact.data(), back.data() + 65536ull * f + lo, hi - lo) == 0, "bytes f=%u lo=%u hi=%u", f,
                          lo, hi);
                    // and at an address of every residue inside a canary frame
                    Bytes wide(64 + (hi - lo), 0xA5);
                    sg.dst = 16 + ((a + e) & 15);
                    CHECK(serve(row, sg, wide.data()), "serve wide");
                    Bytes want(wide.size(), 0xA5);
                    std::memcpy(want.data() + sg.dst, back.data() + 65536ull * f + lo, hi - lo);
                    CHECK(wide == want, "canary f=%u lo=%u hi=%u residue %u", f, lo, hi, (a + e) & 15);
                }
        // a frame that disagrees with the index or its CRC is bad, and nothing is stored
        fread::Seg sg{};
        sg.clen = uint32_t(off[f + 1] - off[f] - 4);
        sg.ulen = ulen;
        sg.hi = 10;
        Bytes out(10, 0xA5);
        fread::Seg wrong = sg;
        wrong.clen += 1;
        CHECK(!serve(row, wrong, out.data()), "wrong clen");
        wrong = sg;
        wrong.ulen -= 1;
        CHECK(!serve(row, wrong, out.data()), "wrong ulen");
        wrong = sg;
        wrong.clen = 3;
        CHECK(!serve(row, wrong, out.data()), "no room");
        Bytes flipped = row;
        flipped[5] ^= 1;
        CHECK(!serve(flipped, sg, out.data()), "crc");
        flipped = row;
        flipped[row.size() / 2] ^= 1;
        CHECK(!serve(flipped, sg, out.data()), "body");
        flipped = row;
        flipped[0] = 0x80;
        CHECK(!serve(flipped, sg, out.data()), "type");
        CHECK(out == Bytes(10, 0xA5), "nothing stored");
    }
    // lane_zero at every residue and length
    for (uint32_t a = 0; a < 16; ++a)
        for (uint32_t len : {0u, 1u, 15u, 16u, 17u, 31u, 100u, 5000u}) {
            Bytes wide(64 + len, 0xA5), want(64 + len, 0xA5);
            for (uint32_t lane = 0; lane < 256; ++lane) fread::lane_zero(wide.data() + 16 + a, len, lane, 256);
            std::memset(want.data() + 16 + a, 0, len);
            CHECK(wide == want, "lane_zero %u %u", a, len);
        }
}

int main() {
    check_walk_and_chain();
    check_store();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
