// fread_plan_check.cpp — the host plan of the frame reads
// (carbonado_amd/csrc/fread_plan.hpp).  Stand-alone: built with ASan + UBSan by
// tests/test_fread_cpu.py and run directly with a seed.
//
//   * the read: request -> frames -> staging rows -> work items over seeded
//     indexes, against a brute-force map that takes every plaintext byte of
//     every request to its frame, its place in the frame, its staging row and
//     its content byte: every content byte is stored by exactly one work item,
//     at the right place, from the right frame.
//   * the index check's header reads: one identifier read and one read per
//     frame, clipped at the stream's end, rows apart.
//   * scratch lengths: multiples of 16 that grow with every number.
//   * the order of the host-decided errors.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/fread_plan.hpp"
#include "plan_shift.hpp"

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

struct Corpus {
    uint64_t ns = 0, shift = 0;
    uint8_t format = 14;
    std::vector<uint32_t> chunk_len, padding;
    std::vector<uint64_t> frame_off, idx_off, nframes, plain_len;
};

static Corpus corpus(std::mt19937_64 &g, uint8_t format) {
    Corpus c;
    c.format = format;
    c.shift = fread::shift_of(format);
    c.ns = 2 + g() % 6;
    uint64_t at = g() % 4;
    c.frame_off.assign(at, 0xDEAD);
    for (uint64_t s = 0; s < c.ns; ++s) {
        const uint64_t nf = s == 0 ? 0 : g() % 6;
        c.idx_off.push_back(at);
        c.nframes.push_back(nf);
        uint64_t pos = nf ? 10 : 0;
        for (uint64_t f = 0; f < nf; ++f) {
            c.frame_off.push_back(pos);
            pos += g() % 5 == 0 ? 1 + g() % 12 : 9 + g() % 70000;  // some without room for a chunk
        }
        c.frame_off.push_back(pos);
        for (uint64_t k = g() % 3; k; --k) c.frame_off.push_back(0xDEAD);
        at = c.frame_off.size();
        c.plain_len.push_back(nf ? 65536 * (nf - 1) + 1 + g() % 65536 : 0);
        const uint64_t obj = pos + c.shift;
        uint64_t C = rules::up((obj + 3) / 4, 1024);
        if (C == 0) C = 1024;
        c.chunk_len.push_back(uint32_t(C));
        c.padding.push_back(uint32_t(4 * C - obj));
        CHECK(fread::stream_len(uint32_t(C), uint32_t(4 * C - obj), c.shift) == pos, "stream_len");
    }
    return c;
}

static void check_read(std::mt19937_64 &g, uint8_t format) {
    const Corpus c = corpus(g, format);
    const uint64_t nreq = 1 + g() % 40;
    std::vector<uint32_t> rs(nreq), kill(c.ns, 0);
    std::vector<uint64_t> start(nreq), len(nreq);
    const bool killing = g() % 2;
    if (killing) kill[1 + g() % (c.ns - 1)] = 11;
    for (uint64_t r = 0; r < nreq; ++r) {
        rs[r] = uint32_t(g() % c.ns);
        const uint64_t P = c.plain_len[rs[r]];
        switch (g() % 6) {
            case 0: start[r] = 0; len[r] = P; break;
            case 1: start[r] = P ? g() % P : 0; len[r] = 0; break;
            case 2: start[r] = P + g() % 3; len[r] = 10; break;
            case 3: start[r] = P ? 65536 * (g() % ((P + 65535) / 65536)) : 0; len[r] = 65536 * (1 + g() % 2); break;
            default: start[r] = P ? g() % P : 0; len[r] = 1 + g() % 140000; break;
        }
    }
    const uint32_t *kp = killing ? kill.data() : nullptr;
    CHECK(fread::check_reads(format, 0, c.chunk_len.data(), c.padding.data(), c.frame_off.data(), c.idx_off.data(),
                             c.nframes.data(), c.plain_len.data(), kp, c.ns, rs.data(), start.data(), len.data(),
                             nreq) == CHIP_OK, "check_reads");
    fread::ReadPlan p;
    fread::plan_ranges(c.chunk_len.data(), c.padding.data(), c.frame_off.data(), c.idx_off.data(), c.plain_len.data(), kp,
                       c.shift, rs.data(), start.data(), len.data(), nreq, &p);
    std::vector<uint64_t> coff(nreq), clen(nreq);
    uint64_t total = 0;
    fread::layout_content(p, 16 * (1 + g() % 3), coff.data(), clen.data(), &total);
    for (uint64_t r = 0; r < nreq; ++r) CHECK(coff[r] % 16 == 0 && (r == 0 || coff[r] >= coff[r - 1] + clen[r - 1]), "layout");
    total = 0;
    for (uint64_t r = 0; r < nreq; ++r) {  // the caller's own offsets: any byte address
        total += 1 + r % 15;
        coff[r] = total;
        total += clen[r];
    }
    fread::plan_items(c.frame_off.data(), c.idx_off.data(), c.nframes.data(), c.plain_len.data(), kp, rs.data(),
                      coff.data(), &p);
    const fread::Req *reqs = reinterpret_cast<const fread::Req *>(p.table.data());
    const fread::Seg *segs = reinterpret_cast<const fread::Seg *>(p.table.data() + nreq * sizeof(fread::Req));
    CHECK(p.table.size() == nreq * sizeof(fread::Req) + p.nseg * sizeof(fread::Seg), "table size");
    // brute force: every plaintext byte of every request
    std::vector<int> stored(total + 32, 0);
    uint64_t stage = 0, nseg = 0, vseg = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        const uint32_t s = rs[r];
        const uint64_t P = c.plain_len[s];
        const uint64_t b = start[r], e = !len[r] || b >= P ? b : (P - b < len[r] ? P : b + len[r]);
        const uint64_t *off = c.frame_off.data() + c.idx_off[s];
        CHECK(clen[r] == e - b && reqs[r].n == e - b && reqs[r].dst == coff[r], "content of %llu", (unsigned long long)r);
        CHECK(reqs[r].kill == (kp ? kp[s] : 0), "kill");
        CHECK(p.vcoff[r] == stage && stage % 16 == 0, "row of %llu", (unsigned long long)r);
        if (e == b || (kp && kp[s])) {
            CHECK(reqs[r].nseg == 0 && p.vlen[r] == 0, "no work for %llu", (unsigned long long)r);
            continue;
        }
        const uint64_t f0 = b / 65536, f1 = (e - 1) / 65536;
        CHECK(p.vstart[r] == c.shift + off[f0] && p.vlen[r] == off[f1 + 1] - off[f0] && p.pos[r] == off[f0], "row range");
        CHECK(reqs[r].seg0 == nseg && reqs[r].nseg == f1 - f0 + 1, "segments of %llu", (unsigned long long)r);
        for (uint64_t x = b; x < e; ++x) {
            const uint64_t f = x / 65536, in = x % 65536;
            const fread::Seg &sg = segs[reqs[r].seg0 + (f - f0)];
            const bool mine = sg.req == r && in >= sg.lo && in < sg.hi && sg.dst + (in - sg.lo) == coff[r] + (x - b);
            if (!mine) {
                CHECK(false, "byte %llu of request %llu", (unsigned long long)x, (unsigned long long)r);
                break;
            }
            ++stored[sg.dst + (in - sg.lo)];
        }
        for (uint64_t f = f0; f <= f1; ++f) {
            const fread::Seg &sg = segs[reqs[r].seg0 + (f - f0)];
            const uint64_t room = off[f + 1] - off[f];
            CHECK(sg.src == stage + (off[f] - off[f0]), "src");
            CHECK(sg.clen == (room >= 8 ? room - 4 : 0), "clen");
            CHECK(sg.ulen == (f + 1 == c.nframes[s] ? P - 65536 * f : 65536) && sg.hi <= sg.ulen && sg.lo < sg.hi, "ulen");
            CHECK(sg.clen < 4 || sg.src + 4 + sg.clen <= stage + p.vlen[r], "the chunk lies inside the row");
            // what the work items store adds up to the range and nothing else
        }
        uint64_t sum = 0;
        for (uint32_t k = 0; k < reqs[r].nseg; ++k) sum += segs[reqs[r].seg0 + k].hi - segs[reqs[r].seg0 + k].lo;
        CHECK(sum == e - b, "the work items of %llu store its range", (unsigned long long)r);
        stage += rules::up16(p.vlen[r]);
        nseg += f1 - f0 + 1;
        vseg += read::range_of(c.chunk_len[s], c.padding[s], p.vstart[r], p.vlen[r]).nseg;
    }
    CHECK(stage == p.stage_total && nseg == p.nseg && vseg == p.vseg, "totals");
    for (int n : stored) CHECK(n <= 1, "a content byte stored twice");
    CHECK(!rules::ranges_overlap(p.vcoff.data(), p.vlen.data(), nreq), "rows apart");
    // the shift case: the plan takes the caller's content offsets and no base (the call adds that on the device);
    // with every offset D higher, every request's and every segment's destination is D higher, nothing else changed
    for (const uint64_t D : plan_shift::SHIFTS) {
        const std::vector<uint64_t> far = plan_shift::moved(coff, D);
        fread::ReadPlan q;
        fread::plan_ranges(c.chunk_len.data(), c.padding.data(), c.frame_off.data(), c.idx_off.data(), c.plain_len.data(), kp,
                           c.shift, rs.data(), start.data(), len.data(), nreq, &q);
        fread::plan_items(c.frame_off.data(), c.idx_off.data(), c.nframes.data(), c.plain_len.data(), kp, rs.data(),
                          far.data(), &q);
        CHECK(q.nseg == p.nseg && q.stage_total == p.stage_total && q.vseg == p.vseg && q.vcoff == p.vcoff, "shifted totals");
        CHECK(plan_shift::shifted_words(p.table, q.table, D) == (long)(nreq + p.nseg), "shifted table");
        const fread::Req *qr = reinterpret_cast<const fread::Req *>(q.table.data());
        const fread::Seg *qs = reinterpret_cast<const fread::Seg *>(q.table.data() + nreq * sizeof(fread::Req));
        for (uint64_t r = 0; r < nreq; ++r) CHECK(qr[r].dst == reqs[r].dst + D, "shifted request");
        for (uint64_t k = 0; k < p.nseg; ++k) CHECK(qs[k].dst == segs[k].dst + D && qs[k].src == segs[k].src, "shifted segment");
        CHECK(rules::ranges_overlap(far.data(), clen.data(), nreq) == rules::ranges_overlap(coff.data(), clen.data(), nreq),
              "overlap verdict");
    }
}

static void check_verify(std::mt19937_64 &g, uint8_t format) {
    const Corpus c = corpus(g, format);
    std::vector<uint64_t> offs;
    std::vector<uint32_t> nfr(c.ns), skip(c.ns, 0);
    std::vector<fread::Geo> geo(c.ns);
    for (uint64_t s = 0; s < c.ns; ++s) {
        nfr[s] = uint32_t(c.nframes[s]);
        for (uint64_t f = 0; f <= c.nframes[s]; ++f) offs.push_back(c.frame_off[c.idx_off[s] + f]);
        geo[s] = fread::geo_of(8ull * c.chunk_len[s], c.chunk_len[s], c.padding[s], c.shift);
        CHECK(geo[s].status == 0 && geo[s].L == offs.back() && geo[s].N == 8 * c.chunk_len[s] / 1024, "geo");
    }
    skip[c.ns - 1] = 17;
    if (c.nframes[1]) offs[1 + 1] = geo[1].L + 5;  // an entry behind the stream: no read, the chain check sees it
    fread::VerifyPlan p;
    fread::plan_verify(offs, nfr, skip, geo, c.shift, &p);
    CHECK(p.nreq == offs.size() && p.table.size() == p.offsets_at + 8 * offs.size(), "sizes");
    uint64_t e = 0;
    for (uint64_t s = 0; s < c.ns; ++s) {
        fread::VStream v;
        std::memcpy(&v, p.table.data() + s * sizeof v, sizeof v);
        CHECK(v.L == geo[s].L && v.ent0 == e && v.nframes == nfr[s] && v.skip == skip[s], "stream %llu", (unsigned long long)s);
        for (uint64_t f = 0; f <= nfr[s]; ++f, ++e) {
            const uint64_t at = f == 0 ? 0 : offs[e - 1], want = f == 0 ? 10 : 12;
            const uint64_t n = skip[s] || at >= v.L ? 0 : std::min(want, v.L - at);
            CHECK(p.req_stream[e] == s && p.coff[e] == 16 * e && p.len[e] == n, "read %llu", (unsigned long long)e);
            if (n) CHECK(p.start[e] == c.shift + at && p.pos[e] == at, "range %llu", (unsigned long long)e);
        }
    }
    CHECK(fread::geo_of(0, 0, 0, 0).status == 0 && fread::geo_of(0, 0, 0, 0).L == 0, "the empty object at 14");
    CHECK(fread::geo_of(8192, 1024, 4097, 0).status == CHIP_ERR_ZFEC, "padding");
    CHECK(fread::geo_of(8192, 2048, 0, 0).status == CHIP_ERR_ZFEC && fread::geo_of(8192, 1000, 0, 0).status == CHIP_ERR_ZFEC,
          "chunk_len");
    CHECK(fread::geo_of(8192, 1024, 4000, 97).L == 0 && fread::geo_of(8192, 1024, 3000, 97).L == 999, "an envelope's stream");
}

static void check_lengths() {
    for (uint64_t ns : {1ull, 3ull, 1024ull})
        for (uint64_t ne : {1ull, 17ull, 20000ull}) {
            const uint64_t s = fread::index_scratch_len(ns, ne);
            CHECK(s % 16 == 0 && s >= 16 * ne + 8 * ne + vread::scratch_len(ne, 2 * ne), "index scratch");
            CHECK(fread::index_scratch_len(ns + 1, ne) > s && fread::index_scratch_len(ns, ne + 2) > s, "grows");
        }
    CHECK(fread::index_scratch_len(1ull << 31, 1) == 0 && fread::index_scratch_len(1, 1ull << 30) == 0, "limits");
    for (uint64_t nreq : {1ull, 40ull, 16384ull})
        for (uint64_t nseg : {1ull, 50ull, 30000ull}) {
            const uint64_t s = fread::read_scratch_len(nreq, nseg, 65536 * nseg, 2 * nreq, 8);
            CHECK(s % 16 == 0 && s >= 65536 * nseg + 32 * nreq + 44 * nseg + vread::scratch_len(nreq, 2 * nreq), "read scratch");
            CHECK(fread::read_scratch_len(nreq + 1, nseg, 65536 * nseg, 2 * nreq, 8) > s, "nreq");
            CHECK(fread::read_scratch_len(nreq, nseg + 4, 65536 * nseg, 2 * nreq, 8) > s, "nseg");
            CHECK(fread::read_scratch_len(nreq, nseg, 65536 * nseg + 16, 2 * nreq, 8) > s, "stage");
            CHECK(fread::read_scratch_len(nreq, nseg, 65536 * nseg, 2 * nreq + 64, 8) > s, "vseg");
            CHECK(fread::read_scratch_len(nreq, nseg, 65536 * nseg, 2 * nreq, 9) > s, "streams");
        }
    CHECK(fread::read_scratch_len(1ull << 31, 1, 16, 1, 1) == 0 && fread::read_scratch_len(1, 1ull << 31, 16, 1, 1) == 0, "limits");
}

static void check_errors() {
    // one stream of two frames at 14: L = 4 * 1024 - 96 = 4000
    const uint32_t cl[1] = {1024}, pad[1] = {96};
    uint64_t fo[3] = {10, 2000, 4000};
    const uint64_t io[1] = {0}, nf[1] = {2}, pl[1] = {65536 + 7};
    const uint32_t rs[2] = {0, 0};
    const uint64_t st[2] = {5, 70000}, ln[2] = {10, 10};
    auto run = [&](uint8_t format, uint32_t flags, const uint64_t *off, const uint64_t *nfr, const uint64_t *plain,
                   const uint32_t *kill, const uint32_t *req_stream, const uint64_t *start, uint64_t nreq, uint64_t ns) {
        return fread::check_reads(format, flags, cl, pad, off, io, nfr, plain, kill, ns, req_stream, start, ln, nreq);
    };
    CHECK(run(14, 0, fo, nf, pl, nullptr, rs, st, 2, 1) == CHIP_OK && run(14, 1, fo, nf, pl, nullptr, rs, st, 2, 1) == CHIP_OK, "ok");
    const uint32_t rs_bad[2] = {0, 1};
    const uint64_t st_bad[2] = {5, (1ull << 53) + 1};
    uint64_t fo_bad[3] = {10, 10, 4000};
    CHECK(run(13, 2, fo_bad, nf, pl, nullptr, rs_bad, st_bad, 1ull << 31, 1) == CHIP_ERR_INVALID_ARG, "format first");
    for (uint8_t f : {0, 12, 13, 16}) CHECK(run(f, 0, fo, nf, pl, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "format");
    for (uint32_t f : {2u, 3u, 1u << 31}) CHECK(run(14, f, fo, nf, pl, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "flags");
    CHECK(run(14, 0, fo, nf, pl, nullptr, rs, st, 1ull << 31, 1) == CHIP_ERR_INVALID_ARG, "nreq");
    CHECK(run(14, 0, fo, nf, pl, nullptr, rs, st, 2, 1ull << 31) == CHIP_ERR_INVALID_ARG, "nstreams");
    CHECK(run(14, 0, fo, nf, pl, nullptr, rs_bad, st, 2, 1) == CHIP_ERR_INVALID_ARG, "req_stream");
    CHECK(run(14, 0, fo, nf, pl, nullptr, rs, st_bad, 2, 1) == CHIP_ERR_INVALID_ARG, "start");
    CHECK(run(14, 0, fo_bad, nf, pl, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "entries that do not ascend");
    fo_bad[1] = 2000;
    fo_bad[2] = 3999;
    CHECK(run(14, 0, fo_bad, nf, pl, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "a last entry that is not L");
    CHECK(run(15, 0, fo, nf, pl, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "L at 15 is 97 less");
    const uint64_t pl_bad[3] = {65536, 2 * 65536 + 1, 0}, nf0[1] = {0};
    for (uint64_t p : pl_bad) CHECK(run(14, 0, fo, nf, &p, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "plain_len");
    CHECK(run(14, 0, fo, nf0, pl_bad + 2, nullptr, rs, st, 2, 1) == CHIP_ERR_INVALID_ARG, "no frame in a stream with bytes");
    const uint32_t kill[1] = {16};
    CHECK(run(14, 0, fo_bad, nf, pl_bad, kill, rs, st, 2, 1) == CHIP_OK, "a killed stream's index is not looked at");
    CHECK(fread::index_fits(fo + 2, 0, 0, 4000) && !fread::index_fits(fo + 2, 0, 1, 4000), "an empty index");
}

int main(int argc, char **argv) {
    std::mt19937_64 g(argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1);
    for (int round = 0; round < 150; ++round) {
        check_read(g, round % 2 ? 15 : 14);
        check_verify(g, round % 2 ? 14 : 15);
    }
    check_lengths();
    check_errors();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
