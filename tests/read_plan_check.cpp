// read_plan_check.cpp — the host logic of the ranged reads
// (carbonado_amd/csrc/read_plan.hpp: argument checks, layout, segments, slice
// requests, fallback items, mask table, scratch layout) driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_read_cpu.py).  No device: the
// addresses are made-up integers, nothing is dereferenced.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/read_plan.hpp"
#include "plan_shift.hpp"

using namespace chip;
using namespace chip::read;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

struct Region {
    uint64_t lo, hi;
};

static void expect_disjoint(std::vector<Region> r, uint64_t limit) {
    std::sort(r.begin(), r.end(), [](const Region &a, const Region &b) { return a.lo < b.lo; });
    for (size_t i = 0; i < r.size(); ++i) {
        EXPECT(r[i].lo <= r[i].hi && r[i].hi <= limit);
        if (i) EXPECT(r[i - 1].hi <= r[i].lo);
    }
}

// all 163 masks with at least 4 bits: sel = the four lowest set bits, and for
// every primary p outside the mask, row p of coef times the selected rows of
// the encoding matrix is e_p; masks with fewer bits are refused
static void check_masks() {
    const Gf256 &g = Gf256::get();
    const std::vector<uint8_t> enc = zfec_enc_matrix(4, 8);
    const std::vector<MaskEntry> &t = mask_table();
    EXPECT(t.size() == 256);
    int usable = 0, rows = 0;
    for (uint32_t m = 0; m < 256; ++m) {
        const MaskEntry &e = t[m];
        if (__builtin_popcount(m) < 4) {
            EXPECT(!e.ok);
            continue;
        }
        ++usable;
        EXPECT(e.ok == 1);
        uint32_t k = 0;
        for (uint32_t i = 0; i < 8 && k < 4; ++i)
            if (m >> i & 1) EXPECT(e.sel[k++] == i);
        EXPECT(k == 4);
        for (uint32_t p = 0; p < 4; ++p) {
            if (m >> p & 1) continue;
            ++rows;
            for (int c = 0; c < 4; ++c) {
                uint8_t acc = 0;
                for (int s = 0; s < 4; ++s) acc ^= g.mul(e.coef[4 * p + s], enc[4 * e.sel[s] + c]);
                EXPECT(acc == (c == (int)p ? 1 : 0));
            }
        }
    }
    EXPECT(usable == 163 && rows > 0);
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    check_masks();
    const uintptr_t IN = 0x10000000, OUT = 0x4000000000, HASH = 0x70000000, SCR = 0x7800000000;
    for (int round = 0; round < 150; ++round) {
        const uint64_t nstreams = 1 + rng() % 12, nreq = 1 + rng() % 60;
        std::vector<uint64_t> in_off(nstreams), in_len(nstreams);
        std::vector<uint32_t> chunk_len(nstreams), padding(nstreams);
        uint64_t cur = 56;
        for (uint64_t s = 0; s < nstreams; ++s) {
            const uint64_t spc = rng() % 5 == 0 ? 1 + rng() % 4096 : 1 + rng() % 9;
            chunk_len[s] = (uint32_t)(1024 * spc);
            padding[s] = (uint32_t)(rng() % 4096);
            in_len[s] = audit::bao_len(8192 * spc);
            in_off[s] = cur;
            cur += up(in_len[s], 256) + 8 * (rng() % 3);
        }
        const uint64_t misfit = rng() % 4 == 0 ? rng() % nstreams : nstreams;  // one stream whose chunk_len does not fit
        if (misfit < nstreams) chunk_len[misfit] += 1024;
        std::vector<uint32_t> req_stream(nreq);
        std::vector<uint64_t> start(nreq), len(nreq), off(nreq), clen(nreq), clen2(nreq);
        for (uint64_t r = 0; r < nreq; ++r) {
            const uint32_t s = (uint32_t)(rng() % nstreams);
            const uint64_t C = chunk_len[s], n_obj = 4 * C - padding[s];
            req_stream[r] = s;
            switch (rng() % 7) {
                case 0: start[r] = 0; len[r] = n_obj + rng() % 3; break;               // the whole object
                case 1: start[r] = n_obj - 1 - rng() % std::min<uint64_t>(3, n_obj); len[r] = 1 + rng() % 9; break;
                case 2: start[r] = n_obj + rng() % 5000; len[r] = 1 + rng() % 100; break;  // in or past the padding
                case 3: start[r] = rng() % n_obj; len[r] = 0; break;
                case 4: start[r] = C * (1 + rng() % 3) - 5; len[r] = 10; break;         // over a primary boundary
                default: start[r] = rng() % n_obj; len[r] = 1 + rng() % (rng() % 2 ? 64 : 3 * C); break;
            }
        }
        const uint64_t align = 16 * (1 + rng() % 20);
        uint64_t total = 0, nseg = 0;
        // layout() knows no stream length: give it the fitting chunk_len and compare where both fit
        EXPECT(layout(chunk_len.data(), padding.data(), nstreams, req_stream.data(), start.data(), len.data(), nreq, align,
                      off.data(), clen.data(), &total, &nseg) == CHIP_OK);
        uint64_t c = 0;
        for (uint64_t r = 0; r < nreq; ++r) {
            EXPECT(off[r] == c && off[r] % align == 0);
            c += up(clen[r], align);
        }
        EXPECT(c == total);
        const uint64_t need = scratch_len(nreq, nseg);
        EXPECT(need % 16 == 0 && scratch_len(nreq + 1, nseg) >= need && scratch_len(nreq, nseg + 1) >= need);
        Plan p;
        EXPECT(plan_read(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                         req_stream.data(), start.data(), len.data(), nreq, OUT, off.data(), clen2.data(), true, SCR, need,
                         &p) == CHIP_OK);
        EXPECT(p.nreq == nreq && p.nseg <= nseg && p.lay.total <= need && p.ka.table.size() == p.lay.table_end);
        const audit::ScratchLayout &ka = p.ka.lay;
        EXPECT(p.ka.nreq == p.nseg);
        expect_disjoint({{p.lay.audit, p.lay.audit + ka.total},
                         {p.lay.masks, p.lay.masks + 256 * sizeof(MaskEntry)},
                         {p.lay.reqs, p.lay.reqs + nreq * sizeof(Req)},
                         {p.lay.segs, p.lay.segs + p.nseg * sizeof(Seg)},
                         {p.lay.fpar, p.lay.fpar + 8 * (p.nseg + 1)},
                         {p.lay.blocks, p.lay.blocks + 8 * (p.nseg + 1)},
                         {p.lay.rstat, p.lay.rstat + 32 * p.nseg},
                         {p.lay.served, p.lay.served + p.nseg * sizeof(Served)}},
                        p.lay.total);
        if (p.nseg) {
            Plan q;
            EXPECT(plan_read(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                             req_stream.data(), start.data(), len.data(), nreq, OUT, off.data(), clen2.data(), true, SCR,
                             p.lay.total - 1, &q) == CHIP_ERR_INVALID_ARG);
        }
        // the shift case: stream and content offsets moved by D, and the two bases moved by D
        for (const uint64_t D : plan_shift::SHIFTS) {
            const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D), off_far = plan_shift::moved(off, D);
            std::vector<uint64_t> len_a(nreq), len_b(nreq);
            Plan by_off, by_base;
            EXPECT(plan_read(IN, in_far.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                             req_stream.data(), start.data(), len.data(), nreq, OUT, off_far.data(), len_a.data(), true,
                             SCR, need, &by_off) == CHIP_OK);
            EXPECT(plan_read(IN + D, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                             req_stream.data(), start.data(), len.data(), nreq, OUT + D, off.data(), len_b.data(), true,
                             SCR, need, &by_base) == CHIP_OK);
            EXPECT(len_a == clen2 && len_b == clen2 && by_off.ka.table == by_base.ka.table);
            EXPECT(by_off.nseg == p.nseg && by_off.total_blocks == p.total_blocks && by_off.fb_parents == p.fb_parents);
            EXPECT(by_off.prim_parents == p.prim_parents && by_off.prim_chunks == p.prim_chunks);
            // per segment: the stream's address twice (the segment, its slice request) and the content address
            EXPECT(plan_shift::shifted_words(p.ka.table, by_off.ka.table, D) == (long)(3 * p.nseg));
            for (uint64_t k = 0; k < p.nseg; ++k) {
                EXPECT(by_off.segs()[k].src == p.segs()[k].src + D && by_off.segs()[k].dst == p.segs()[k].dst + D);
                EXPECT(by_off.ka.reqs()[k].src == p.ka.reqs()[k].src + D && by_off.ka.reqs()[k].hash == p.ka.reqs()[k].hash);
            }
            EXPECT(audit::ranges_overlap(off_far.data(), clen2.data(), nreq) == audit::ranges_overlap(off.data(), clen2.data(), nreq));
        }
        uint64_t g = 0;
        const uint64_t *parents = p.ka.parents(), *chunks = p.ka.chunks();
        for (uint64_t r = 0; r < nreq; ++r) {
            const uint32_t s = req_stream[r];
            const Req &rq = p.reqs()[r];
            if (s == misfit) {
                EXPECT(rq.status == CHIP_ERR_ZFEC && rq.nseg == 0 && clen2[r] == 0);
                continue;
            }
            const uint64_t C = chunk_len[s], spc = C / 1024, n_obj = 4 * C - padding[s];
            const uint64_t want = start[r] < n_obj && len[r] ? std::min(n_obj, start[r] + len[r]) - start[r] : 0;
            EXPECT(rq.status == 0 && clen2[r] == want && clen[r] == want && rq.seg0 == g);
            EXPECT(want ? rq.nseg >= 1 && rq.nseg <= 4 : rq.nseg == 0);
            // the segments tile the request's object range exactly once, in order
            uint64_t x = start[r], dst = OUT + off[r];
            for (uint32_t k = 0; k < rq.nseg; ++k, ++g) {
                const Seg &sg = p.segs()[g];
                EXPECT(sg.req == r && sg.src == IN + in_off[s] && sg.N == 8 * spc && sg.spc == spc && sg.p < 4);
                EXPECT(sg.c0 < sg.c1 && sg.c1 <= C && sg.p * C + sg.c0 == x && sg.dst == dst);
                if (k) EXPECT(sg.c0 == 0 && sg.p == p.segs()[g - 1].p + 1 && p.segs()[g - 1].c1 == C);
                const uint64_t w0 = sg.c0 / 1024, w1 = (sg.c1 + 1023ull) / 1024;
                EXPECT(w0 * 1024 <= sg.c0 && sg.c1 <= w1 * 1024 && w1 <= spc && w1 - w0 <= (sg.c1 - sg.c0 + 2046ull) / 1024);
                // its own slice request: the window of primary p; the 7 fallbacks are that record moved by
                // whole shards, their parent items 7 x the most any of them selects
                const audit::Req &a = p.ka.reqs()[g];
                EXPECT(a.src == sg.src && a.hash == HASH + 32 * s && a.n == 8 * C && a.N == sg.N && a.olen == 0);
                EXPECT(a.first == sg.p * spc + w0 && a.last == sg.p * spc + w1);
                EXPECT(chunks[g + 1] - chunks[g] == w1 - w0);
                EXPECT(parents[g + 1] - parents[g] == audit::sel_parents(a.N, a.first, a.last));
                uint64_t most = 0, words = 0;
                for (uint32_t i = 0; i < 8; ++i) {
                    const uint64_t j = status_word(p.nseg, g, sg.p, i);
                    EXPECT(i == sg.p ? j == g : j >= p.nseg && j < 8 * p.nseg && (j - p.nseg) / 7 == g);
                    words |= 1ull << (i == sg.p ? 7 : (j - p.nseg) % 7);
                    if (i != sg.p) most = std::max(most, audit::sel_parents(a.N, i * spc + w0, i * spc + w1));
                }
                EXPECT(words == 0xFF && most >= 1 && p.fpar()[g + 1] - p.fpar()[g] == 7 * most);
                const uint64_t bytes = sg.c1 - sg.c0, nb = p.blocks()[g + 1] - p.blocks()[g];
                EXPECT(nb * BLOCK >= bytes + dst % 16 && (nb - 1) * BLOCK < bytes + dst % 16);
                x += bytes;
                dst += bytes;
            }
            EXPECT(x == start[r] + want);
        }
        EXPECT(g == p.nseg && p.blocks()[0] == 0 && p.blocks()[p.nseg] == p.total_blocks);
        EXPECT(p.prim_parents == parents[p.nseg] && p.prim_chunks == chunks[p.nseg]);
        EXPECT(p.fpar()[0] == 0 && p.fb_parents == p.fpar()[p.nseg]);
        if (misfit == nstreams) EXPECT(p.nseg == nseg);
    }
    // call-level refusals, in the header's order
    {
        const uint64_t len2[2] = {audit::bao_len(8192), audit::bao_len(8192 * 5)}, off2[2] = {56, 65536 + 8};
        const uint32_t cl[2] = {1024, 5120}, pad[2] = {1, 2}, rs[3] = {0, 1, 1};
        const uint64_t st[3] = {0, 5000, 100}, ln[3] = {100, 9000, 0}, co[3] = {0, 112, 9120};
        uint64_t out[3];
        const uint64_t need = scratch_len(3, 4);
        auto call = [&](uintptr_t in, const uint64_t *io, const uint64_t *il, uintptr_t hash, const uint32_t *r,
                        const uint64_t *s, uintptr_t content, const uint64_t *o, uintptr_t scr, uint64_t sl,
                        uint64_t nreq = 3) {
            Plan p;
            return plan_read(in, io, il, hash, pad, cl, 2, r, s, ln, nreq, content, o, out, true, scr, sl, &p);
        };
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, co, SCR, need) == CHIP_OK);
        EXPECT(out[0] == 100 && out[1] == 9000 && out[2] == 0);
        EXPECT(call(0, off2, len2, HASH, rs, st, OUT, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off2, len2, HASH, rs, st, 0, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, co, 0, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, co, SCR, need, 1ull << 31) == CHIP_ERR_INVALID_ARG);
        const uint32_t rs9[3] = {0, 2, 1};
        EXPECT(call(IN, off2, len2, HASH, rs9, st, OUT, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        const uint64_t stbig[3] = {0, (1ull << 53) + 1, 100};
        EXPECT(call(IN, off2, len2, HASH, rs, stbig, OUT, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        const uint64_t off4[2] = {60, 65536 + 8};
        EXPECT(call(IN, off4, len2, HASH, rs, st, OUT, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        const uint64_t co8[3] = {0, 120, 9120};
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, co8, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, co, SCR + 8, need) == CHIP_ERR_INVALID_ARG);
        const uint64_t lap[3] = {0, 96, 9120};
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, lap, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off2, len2, HASH, rs, st, OUT, co, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
        const uint64_t gap[2] = {len2[0] + 8, len2[1]};
        EXPECT(call(IN, off2, gap, HASH, rs, st, OUT, co, SCR, need) == CHIP_ERR_BAO_TRUNCATED);
        EXPECT(call(IN, off2, gap, 0, rs, st, OUT, co, SCR, need) == CHIP_ERR_BAO_TRUNCATED);
        EXPECT(call(IN, off2, gap, HASH, rs, st, OUT, co8, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off2, len2, 0, rs, st, OUT, co, SCR, need) == CHIP_ERR_HASH_DECODE);
        EXPECT(call(0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 0, 0) == CHIP_OK);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
