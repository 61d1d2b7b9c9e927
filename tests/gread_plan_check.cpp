// gread_plan_check.cpp — the device-planned plaintext reads of level-14 and
// level-15 objects (carbonado_amd/csrc/gread_device.hpp, the text
// gread_kernels.hip runs, compiled here as host code, and gread_plan.hpp, the
// host's O(1) share) driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_gread_cpu.py).  No device: the
// addresses are made-up integers.
//
//  * the frame table: over seeded streams and indexes gread::plan_table accepts
//    what fread::check_reads accepts, its records and compacted entries are
//    where TableLayout says, max_frame is the brute-force maximum, a killed
//    stream has no entries, and a broken index is refused with nothing made;
//  * the rewrite: over seeded requests gread::decide's decision (refused,
//    killed, read), clipped range and frame-stream request are what
//    fread::plan_ranges gives that request; a lying nentries, max_frame or
//    max_chunks refuses exactly the requests it contradicts;
//  * the work items: for every (r, k) of a batch gread::item_of_request equals
//    fread::plan_items' Seg field for field (the staging offset relative to the
//    request's slot), every touched frame fits the slot, and k < fcap;
//  * fcap against a brute-force count of touched frames for every max_len in
//    1..200000 at the worst alignment, and at seeded alignments;
//  * the host checks of a read call in their order and the scratch layout.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/gread_plan.hpp"
#include "plan_shift.hpp"

using namespace chip;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

static const uintptr_t IN = 0x10000000, OUT = 0x4000000000, HASH = 0x70000000, SCR = 0x7800000000, TAB = 0x7900000000,
                       KEYS = 0x7A00000000, FTAB = 0x7B00000000;
static const uint64_t FRAME = fread::FRAME, MAXF = FRAME + 8;

struct World {
    uint8_t format;
    uint64_t ns;
    std::vector<uint64_t> in_off, in_len, frame_off, idx_off, nframes, plain_len;
    std::vector<uint32_t> chunk_len, padding, istat, kstat;
    std::vector<uint8_t> table, ftable;
    chipq_table_info info;
    chipg_frame_info finfo;
    const qread::StreamRec *recs() const { return reinterpret_cast<const qread::StreamRec *>(table.data()); }
    const gread::FrameRec *frecs() const { return reinterpret_cast<const gread::FrameRec *>(ftable.data()); }
    const uint64_t *ent() const {
        return reinterpret_cast<const uint64_t *>(ftable.data() + gread::TableLayout(ns, finfo.nentries).entries);
    }
};

static World make_world(std::mt19937_64 &rng, uint8_t format) {
    World w;
    w.format = format;
    const uint64_t shift = fread::shift_of(format), ns = w.ns = 6 + rng() % 4;
    w.in_off.resize(ns); w.in_len.resize(ns); w.idx_off.resize(ns); w.nframes.resize(ns); w.plain_len.resize(ns);
    w.chunk_len.resize(ns); w.padding.resize(ns);
    w.istat.assign(ns, 0); w.kstat.assign(ns, 0);
    uint64_t cur = 56;
    for (uint64_t s = 0; s < ns; ++s) {
        const uint64_t nf = s == 0 ? 0 : s == 1 ? 1 : 1 + rng() % 5;
        std::vector<uint64_t> off;
        uint64_t L = nf ? 10 : (s % 2 ? 10 : 0);
        for (uint64_t f = 0; f < nf; ++f) {
            off.push_back(L);
            const unsigned kind = rng() % 4;
            L += kind == 0 ? MAXF : kind == 1 ? 8 + rng() % 9 : 9 + rng() % (MAXF - 9);  // raw full, tiny, anything
        }
        off.push_back(L);  // the last entry; the only one of a stream without a frame
        w.nframes[s] = nf;
        w.plain_len[s] = nf ? FRAME * (nf - 1) + (s % 3 == 0 ? FRAME : 1 + rng() % FRAME) : 0;
        const uint64_t C = rules::up(std::max<uint64_t>(L + shift, 1), 4096) / 4;
        w.chunk_len[s] = uint32_t(C);
        w.padding[s] = uint32_t(4 * C - shift - L);
        w.in_off[s] = cur;
        w.in_len[s] = audit::bao_len(8 * C);
        cur += audit::up(w.in_len[s], 8) + 8 * (rng() % 4);
        w.idx_off[s] = w.frame_off.size() + rng() % 3;
        w.frame_off.resize(w.idx_off[s], 0x7777777777ull);
        w.frame_off.insert(w.frame_off.end(), off.begin(), off.end());
    }
    w.frame_off.push_back(0x7777777777ull);
    EXPECT(qread::plan_table(IN, w.in_off.data(), w.in_len.data(), HASH, w.padding.data(), w.chunk_len.data(), ns, TAB,
                             qread::table_len(ns), &w.info, &w.table) == CHIP_OK);
    return w;
}

static int make_ftable(World &w, uint64_t len = ~0ull) {
    return gread::plan_table(w.format, w.chunk_len.data(), w.padding.data(), w.istat.data(), w.frame_off.data(),
                             w.idx_off.data(), w.nframes.data(), w.plain_len.data(), w.ns, FTAB, len, &w.finfo, &w.ftable);
}

// ---- the frame table -------------------------------------------------------------------
static void check_table(std::mt19937_64 &rng) {
    for (int round = 0; round < 40; ++round) {
        World w = make_world(rng, round % 2 ? 15 : 14);
        const uint64_t ns = w.ns;
        if (round % 3 == 0) {
            w.istat[3] = 11;
            for (uint64_t f = 0; f <= w.nframes[3]; ++f) w.frame_off[w.idx_off[3] + f] = 0;  // not looked at
        }
        EXPECT(fread::check_reads(w.format, 0, w.chunk_len.data(), w.padding.data(), w.frame_off.data(), w.idx_off.data(),
                                  w.nframes.data(), w.plain_len.data(), w.istat.data(), ns, nullptr, nullptr, nullptr,
                                  0) == CHIP_OK);
        EXPECT(make_ftable(w) == CHIP_OK);
        uint64_t ne = 0, max_frame = 0;
        for (uint64_t s = 0; s < ns; ++s) {
            if (w.istat[s]) continue;
            ne += w.nframes[s] + 1;
            for (uint64_t f = 0; f < w.nframes[s]; ++f)
                max_frame = std::max(max_frame, w.frame_off[w.idx_off[s] + f + 1] - w.frame_off[w.idx_off[s] + f]);
        }
        EXPECT(w.finfo.nstreams == ns && w.finfo.nentries == ne && w.finfo.max_frame == max_frame &&
               w.finfo.format == w.format);
        const gread::TableLayout lay(ns, ne);
        EXPECT(lay.recs == 0 && lay.entries == 32 * ns && lay.total == 32 * ns + fread::up16(8 * ne));
        EXPECT(w.ftable.size() == lay.total && lay.total == gread::table_len(ns, ne) && lay.total % 16 == 0);
        uint64_t e = 0;
        for (uint64_t s = 0; s < ns; ++s) {
            const gread::FrameRec &r = w.frecs()[s];
            EXPECT(r.plain_len == w.plain_len[s] && r.index_status == w.istat[s] && r.pad_ == 0);
            if (w.istat[s]) {
                EXPECT(r.ent0 == 0 && r.nframes == 0);
                continue;
            }
            EXPECT(r.ent0 == e && r.nframes == w.nframes[s]);
            for (uint64_t f = 0; f <= w.nframes[s]; ++f) EXPECT(w.ent()[e + f] == w.frame_off[w.idx_off[s] + f]);
            e += w.nframes[s] + 1;
        }
        // the length, and a bound of it
        EXPECT(make_ftable(w, lay.total) == CHIP_OK && make_ftable(w, lay.total - 1) == CHIP_ERR_INVALID_ARG);
        EXPECT(w.ftable.empty() && w.finfo.nstreams == 0 && w.finfo.format == 0);
        // a broken index is refused as the host-planned call refuses it
        const uint64_t s = 2, at = w.idx_off[s] + rng() % (w.nframes[s] + 1);
        const uint64_t keep = w.frame_off[at];
        w.frame_off[at] = at == w.idx_off[s] + w.nframes[s] ? keep + 1 : w.frame_off[at + 1];
        EXPECT(fread::check_reads(w.format, 0, w.chunk_len.data(), w.padding.data(), w.frame_off.data(), w.idx_off.data(),
                                  w.nframes.data(), w.plain_len.data(), w.istat.data(), ns, nullptr, nullptr, nullptr,
                                  0) == CHIP_ERR_INVALID_ARG);
        EXPECT(make_ftable(w) == CHIP_ERR_INVALID_ARG && w.ftable.empty() && w.finfo.nentries == 0);
        w.frame_off[at] = keep;
        const uint64_t pl = w.plain_len[1];
        w.plain_len[1] = FRAME + 1;  // one frame cannot hold it
        EXPECT(make_ftable(w) == CHIP_ERR_INVALID_ARG);
        w.plain_len[1] = pl;
        EXPECT(make_ftable(w) == CHIP_OK);
    }
    // the argument checks, in their order
    World w = make_world(rng, 14);
    chipg_frame_info fi;
    std::vector<uint8_t> t;
    const auto rc = [&](uint8_t fmt, bool cl, bool fo, uint64_t ns, uintptr_t tab, uint64_t len, chipg_frame_info *f) {
        return gread::plan_table(fmt, cl ? w.chunk_len.data() : nullptr, w.padding.data(), nullptr,
                                 fo ? w.frame_off.data() : nullptr, w.idx_off.data(), w.nframes.data(),
                                 w.plain_len.data(), ns, tab, len, f, &t);
    };
    EXPECT(rc(14, true, true, w.ns, FTAB, ~0ull, &fi) == CHIP_OK && fi.nstreams == w.ns);
    EXPECT(rc(14, true, true, w.ns, FTAB, ~0ull, nullptr) == CHIP_ERR_INVALID_ARG);
    EXPECT(rc(13, true, true, 0, FTAB, ~0ull, &fi) == CHIP_ERR_INVALID_ARG && fi.format == 0);
    EXPECT(rc(15, false, false, 0, 0, 0, &fi) == CHIP_OK && fi.format == 15 && fi.nstreams == 0 && t.empty());
    EXPECT(rc(14, false, true, w.ns, FTAB, ~0ull, &fi) == CHIP_ERR_INVALID_ARG);
    EXPECT(rc(14, true, false, w.ns, FTAB, ~0ull, &fi) == CHIP_ERR_INVALID_ARG);
    EXPECT(rc(14, true, true, w.ns, 0, ~0ull, &fi) == CHIP_ERR_INVALID_ARG);
    EXPECT(rc(14, true, true, 1ull << 31, FTAB, ~0ull, &fi) == CHIP_ERR_INVALID_ARG);
    EXPECT(rc(14, true, true, w.ns, FTAB + 8, ~0ull, &fi) == CHIP_ERR_INVALID_ARG && fi.nstreams == 0);
    EXPECT(gread::table_len(1ull << 31, 1) == 0 && gread::table_len(1, 1ull << 30) == 0 && gread::table_len(0, 0) == 0);
    EXPECT(gread::table_len(3, 7) == 96 + 64 && gread::table_len(3, 8) == 96 + 64 && gread::table_len(3, 9) == 96 + 80);
}

// ---- the rewrite and the work items ----------------------------------------------------
struct R { uint32_t s; uint64_t start, len; };

static std::vector<R> make_requests(const World &w, std::mt19937_64 &rng, uint64_t max_len) {
    std::vector<R> rq;
    for (uint32_t s = 0; s < w.ns; ++s) {
        const uint64_t P = w.plain_len[s];
        rq.push_back({s, 0, max_len}); rq.push_back({s, 0, 0}); rq.push_back({s, P, 1}); rq.push_back({s, P + 9, max_len});
        rq.push_back({s, P ? P - 1 : 0, 1}); rq.push_back({s, P ? P - 1 : 0, max_len + 9});
        rq.push_back({s, P > max_len ? P - max_len : 0, max_len + 3});                     // clipped to max_len or less
        rq.push_back({s, P > max_len ? P - max_len - 1 : 0, max_len + 3});                 // to max_len + 1 where P allows
        for (uint64_t f = 1; f <= w.nframes[s]; ++f) {
            const uint64_t half = std::min<uint64_t>(max_len / 2, FRAME);
            rq.push_back({s, FRAME * f - std::min<uint64_t>(max_len, FRAME), std::min<uint64_t>(max_len, FRAME)});
            rq.push_back({s, FRAME * f, max_len}); rq.push_back({s, FRAME * f - half, max_len});
            rq.push_back({s, FRAME * f - 1, max_len});
        }
        for (int k = 0; k < 12; ++k) rq.push_back({s, P ? rng() % P : 0, 1 + rng() % max_len});
    }
    rq.push_back({uint32_t(w.ns), 0, 1}); rq.push_back({~0u, 0, 1});
    rq.push_back({1, (1ull << 53) + 1, 1}); rq.push_back({1, 0, (1ull << 53) + 1}); rq.push_back({1, 1ull << 53, 1ull << 53});
    return rq;
}

static void check_rewrite(std::mt19937_64 &rng) {
    const uint64_t lens[] = {1, 4096, 65537, 70000};
    uint64_t seen[4] = {0, 0, 0, 0}, multi = 0;
    for (int round = 0; round < 48; ++round) {
        World w = make_world(rng, round % 2 ? 15 : 14);
        const uint64_t shift = fread::shift_of(w.format), max_len = lens[(round / 2) % 4];
        if (round % 3 == 1) w.istat[2] = 5, w.istat[4] = 11;
        if (w.format == 15 && round % 4 == 3) w.kstat[5] = 17;
        EXPECT(make_ftable(w) == CHIP_OK);
        const std::vector<R> rq = make_requests(w, rng, max_len);
        const uint64_t nreq = rq.size(), cstride = fread::up16(max_len) + 16;
        const gread::Geometry g(w.info, w.finfo, nreq, max_len);
        EXPECT(g.ok && g.fcap == gread::fcap_of(max_len) && g.stage_stride % 16 == 0 &&
               g.inner_len == std::max<uint64_t>(1, g.fcap * w.finfo.max_frame) && g.work == nreq * g.fcap);
        const gread::Shape sh = gread::shape_of(w.info, w.finfo, max_len, g);
        gread::Shape few = sh, shortf = sh, chunks = sh;
        few.nentries -= 1;
        shortf.max_frame -= 1;
        chunks.inner.max_chunks -= 1;
        uint64_t last_live = 0;
        for (uint64_t s = 0; s < w.ns; ++s)
            if (!w.istat[s]) last_live = s;

        // the host plan of the requests it accepts, as one batch at r * cstride
        std::vector<uint32_t> hs;
        std::vector<uint64_t> hstart, hlen, hcoff;
        std::vector<uint64_t> host_of(nreq, ~0ull);
        for (uint64_t r = 0; r < nreq; ++r) {
            if (rq[r].s >= w.ns || rq[r].start > read::MAX_RANGE || rq[r].len > read::MAX_RANGE) continue;
            host_of[r] = hs.size();
            hs.push_back(rq[r].s); hstart.push_back(rq[r].start); hlen.push_back(rq[r].len); hcoff.push_back(r * cstride);
        }
        EXPECT(fread::check_reads(w.format, 0, w.chunk_len.data(), w.padding.data(), w.frame_off.data(), w.idx_off.data(),
                                  w.nframes.data(), w.plain_len.data(), w.istat.data(), w.ns, hs.data(), hstart.data(),
                                  hlen.data(), hs.size()) == CHIP_OK);
        fread::ReadPlan p;
        fread::plan_ranges(w.chunk_len.data(), w.padding.data(), w.frame_off.data(), w.idx_off.data(), w.plain_len.data(),
                           w.istat.data(), shift, hs.data(), hstart.data(), hlen.data(), hs.size(), &p);
        fread::plan_items(w.frame_off.data(), w.idx_off.data(), w.nframes.data(), w.plain_len.data(), w.istat.data(),
                          hs.data(), hcoff.data(), &p);
        const fread::Req *hreq = reinterpret_cast<const fread::Req *>(p.table.data());
        const fread::Seg *hseg = reinterpret_cast<const fread::Seg *>(p.table.data() + hs.size() * sizeof(fread::Req));

        for (uint64_t r = 0; r < nreq; ++r) {
            const gread::Decision d = gread::decide(w.recs(), w.frecs(), w.ent(), w.kstat.data(), sh, rq[r].s, rq[r].start,
                                                    rq[r].len);
            const uint64_t h = host_of[r];
            const uint64_t n = h == ~0ull ? 0 : p.end[h] - p.begin[h];
            if (h == ~0ull || n > max_len) {
                EXPECT(d.order == gread::REFUSED && d.q_stream == gread::NO_STREAM && d.q_len == 0 && d.n == 0);
                ++seen[0];
                continue;
            }
            const uint32_t s = rq[r].s;
            EXPECT(d.q_stream == s && d.n == n && (n == 0 || d.b == p.begin[h]));
            EXPECT(hreq[h].n == n && hreq[h].dst == r * cstride && hreq[h].kill == w.istat[s]);
            if (w.istat[s]) {
                EXPECT(d.order == gread::KILLED && d.kill == w.istat[s] && d.q_len == 0 && d.q_start == 0 && d.nfr == 0);
                EXPECT(hreq[h].nseg == 0);
                ++seen[1];
                continue;
            }
            EXPECT(d.order == gread::READ);
            // the frame-stream request: the vouched read's request in object bytes, the keystream's position
            EXPECT(d.q_len == p.vlen[h] && d.nfr == hreq[h].nseg);
            EXPECT(n == 0 ? d.q_start == 0 && d.q_len == 0 : d.q_start + shift == p.vstart[h] && d.q_start == p.pos[h]);
            EXPECT(d.q_len <= g.inner_len && d.nfr <= g.fcap);
            ++seen[n ? 3 : 2];
            multi += d.nfr == g.fcap && g.fcap > 1;
            const gread::FrameRec &fr = w.frecs()[s];
            bool full = false;
            for (uint32_t k = 0; k < d.nfr; ++k) {
                const fread::Seg mine = gread::item_of_request(fr, w.ent(), d, r, k, g.stage_stride, cstride);
                const fread::Seg &want = hseg[hreq[h].seg0 + k];
                EXPECT(mine.src - r * g.stage_stride == want.src - p.vcoff[h] && mine.dst == want.dst && mine.req == r &&
                       want.req == h && mine.clen == want.clen && mine.ulen == want.ulen && mine.lo == want.lo &&
                       mine.hi == want.hi && mine.pad_ == 0);
                // the frame lies in the request's slot, the stores in its content
                const uint64_t room = w.ent()[fr.ent0 + d.f0 + k + 1] - w.ent()[fr.ent0 + d.f0 + k];
                EXPECT(mine.src - r * g.stage_stride + room <= d.q_len && d.q_len <= g.stage_stride);
                EXPECT(mine.dst >= r * cstride && mine.dst + (mine.hi - mine.lo) <= r * cstride + n && mine.hi <= mine.ulen &&
                       mine.ulen <= FRAME);
                full |= room == w.finfo.max_frame;
            }
            // lying tables refuse exactly the requests they contradict
            const auto order = [&](const gread::Shape &x) {
                return gread::decide(w.recs(), w.frecs(), w.ent(), w.kstat.data(), x, s, rq[r].start, rq[r].len).order;
            };
            EXPECT(order(few) == (s == last_live ? gread::REFUSED : gread::READ));
            EXPECT(order(shortf) == (full ? gread::REFUSED : gread::READ));
            EXPECT(order(chunks) == (w.recs()[s].N == w.info.max_chunks ? gread::REFUSED : gread::READ));
        }
    }
    EXPECT(seen[0] > 100 && seen[1] > 100 && seen[2] > 100 && seen[3] > 1000 && multi > 20);
}

// ---- fcap -----------------------------------------------------------------------------
static void check_fcap(std::mt19937_64 &rng) {
    for (uint64_t len = 1; len <= 200000; ++len) {
        const uint64_t worst = (FRAME - 1 + len - 1) / FRAME + 1;  // a range that starts at a frame's last byte
        EXPECT(gread::fcap_of(len) == worst);
        const uint64_t a = rng() % (4 * FRAME), touched = (a + len - 1) / FRAME - a / FRAME + 1;
        EXPECT(touched <= worst);
    }
    EXPECT(gread::fcap_of(1) == 1 && gread::fcap_of(2) == 2 && gread::fcap_of(4096) == 2 && gread::fcap_of(65537) == 2 &&
           gread::fcap_of(65538) == 3 && gread::fcap_of(70000) == 3);
}

// ---- the host checks of a read call and its scratch ----------------------------------
static void check_call(std::mt19937_64 &rng) {
    World w = make_world(rng, 15);
    EXPECT(make_ftable(w) == CHIP_OK);
    chipg_frame_info f14 = w.finfo;
    f14.format = 14;
    const uint64_t klen = kread::table_len(w.ns);
    const chipg_frame_info *const both[] = {&w.finfo, &f14};
    for (const chipg_frame_info *fi : both) {
        const bool keyed = fi->format == 15;
        const uint64_t nreq = 65, max_len = 4096, need = gread::scratch_len(&w.info, fi, nreq, max_len);
        gread::Geometry g;
        gread::ScratchLayout lay;
        struct A {
            uintptr_t table = TAB, ftab = FTAB, keytab = KEYS, content = OUT, scratch = SCR;
            uint64_t keytab_len, nreq = 65, max_len = 4096, stride = 4096, scratch_len;
            bool info = true, finfo = true, reqs = true, results = true;
            uint32_t flags = 0;
        };
        const auto rc = [&](const A &a, const chipg_frame_info *f) {
            return gread::plan_call(a.table, a.info ? &w.info : nullptr, a.ftab, a.finfo ? f : nullptr, a.keytab,
                                    a.keytab_len, a.reqs, a.nreq, a.max_len, a.content, a.stride, a.results, a.flags,
                                    a.scratch, a.scratch_len, &g, &lay);
        };
        A ok;
        ok.keytab_len = klen;
        ok.scratch_len = need;
        EXPECT(need && need % 16 == 0 && rc(ok, fi) == CHIP_OK && lay.total == need);
        // the shift case: the frame table holds offsets into frame streams and no address, and the stream table is
        // qread's (tests/qread_plan_check.cpp); what a call takes is the content base and stride, past 2^32 here
        for (const uint64_t D : plan_shift::SHIFTS) {
            A far = ok;
            far.content = OUT + D;
            EXPECT(rc(far, fi) == CHIP_OK && lay.total == need);
            far = ok;
            far.stride = D + 256;
            EXPECT(rc(far, fi) == CHIP_OK && lay.total == need);
            far.stride = D + 264;  // no multiple of 16, at any height
            EXPECT(rc(far, fi) == CHIP_ERR_INVALID_ARG);
        }
        EXPECT(rc(ok, fi) == CHIP_OK && lay.total == need);
        // the layout: the inner scratch first, every region on a 256-B boundary, one after another
        const uint64_t inner = keyed ? kread::scratch_len(&w.info, nreq, g.inner_len)
                                     : qread::scratch_len(&w.info, nreq, g.inner_len, true);
        EXPECT(lay.inner == 0 && lay.inner_len == inner && lay.q_stream == read::up(inner, 256));
        EXPECT(lay.q_start == lay.q_stream + read::up(4 * nreq, 256) && lay.q_len == lay.q_start + read::up(8 * nreq, 256) &&
               lay.q_clen == lay.q_len + read::up(8 * nreq, 256) && lay.bad == lay.q_clen + read::up(8 * nreq, 256) &&
               lay.stage == lay.bad + read::up(4 * nreq * g.fcap, 256) && lay.total == lay.stage + nreq * g.stage_stride);
        EXPECT(lay.stage % 256 == 0 && g.stage_stride == fread::up16(2 * w.finfo.max_frame));
        EXPECT(gread::scratch_len(&w.info, fi, nreq + 1, max_len) > need && gread::scratch_len(&w.info, fi, nreq, 70000) > need);
        A a = ok; a.nreq = 0; a.table = 0; a.info = false; a.scratch = 0; a.max_len = 0;
        EXPECT(rc(a, fi) == CHIP_OK);
        a = ok; a.table = 0; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.info = false; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.ftab = 0; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.finfo = false; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.reqs = false; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.results = false; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.content = 0; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.scratch = 0; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.keytab = 0; EXPECT(rc(a, fi) == (keyed ? CHIP_ERR_INVALID_ARG : CHIP_OK));   // counts at 15 only
        a = ok; a.keytab_len = klen - 1; EXPECT(rc(a, fi) == (keyed ? CHIP_ERR_INVALID_ARG : CHIP_OK));
        chipg_frame_info bad = *fi;
        bad.format = 13; EXPECT(rc(ok, &bad) == CHIP_ERR_INVALID_ARG && gread::scratch_len(&w.info, &bad, nreq, max_len) == 0);
        bad = *fi; bad.nstreams += 1;
        EXPECT(rc(ok, &bad) == CHIP_ERR_INVALID_ARG && gread::scratch_len(&w.info, &bad, nreq, max_len) == 0);
        a = ok; a.nreq = 1ull << 31; a.scratch_len = ~0ull; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.max_len = 0; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.max_len = 4097; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);   // the stride is too short
        a = ok; a.stride = 4088; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.content = OUT + 8; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.scratch = SCR + 8; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.table = TAB + 8; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.ftab = FTAB + 8; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.flags = 2; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.flags = 1; EXPECT(rc(a, fi) == CHIP_OK);
        a = ok; a.scratch_len = need - 1; EXPECT(rc(a, fi) == CHIP_ERR_INVALID_ARG);
        a = ok; a.stride = 8192; EXPECT(rc(a, fi) == CHIP_OK);
        // bounds: the inner capacity above 2^53, 2^31 block workgroups, where the outer capacity still passes
        bad = *fi; bad.max_frame = 1ull << 53;
        EXPECT(gread::scratch_len(&w.info, &bad, nreq, max_len) == 0);
        a = ok; a.scratch_len = ~0ull; EXPECT(rc(a, &bad) == CHIP_ERR_INVALID_ARG);
        EXPECT(gread::scratch_len(&w.info, fi, 1 << 20, 1 << 28) == 0);
        EXPECT(gread::scratch_len(nullptr, fi, nreq, max_len) == 0 && gread::scratch_len(&w.info, nullptr, nreq, max_len) == 0 &&
               gread::scratch_len(&w.info, fi, nreq, 0) == 0 && gread::scratch_len(&w.info, fi, 1ull << 31, max_len) == 0);
        // a table without a frame serves its empty and killed requests: an inner capacity of one byte
        bad = *fi; bad.max_frame = 0;
        const gread::Geometry g0(w.info, bad, nreq, max_len);
        EXPECT(g0.ok && g0.inner_len == 1 && g0.stage_stride == 16 && gread::scratch_len(&w.info, &bad, nreq, max_len) > 0);
    }
}

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1);
    check_table(rng);
    check_rewrite(rng);
    check_fcap(rng);
    check_call(rng);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
