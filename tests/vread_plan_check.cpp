// vread_plan_check.cpp — the host logic of the vouched ranged reads
// (carbonado_amd/csrc/vread_plan.hpp: the extra argument checks, the scratch
// layout behind a ranged read's, the vouch items) driven stand-alone, for a
// build with -fsanitize=address,undefined (tests/test_vread_cpu.py).  No
// device: the addresses are made-up integers, nothing is dereferenced.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "../carbonado_amd/csrc/vread_plan.hpp"
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

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    const uintptr_t IN = 0x10000000, OUT = 0x4000000000, HASH = 0x70000000, SCR = 0x7800000000;
    uint64_t items_seen = 0;
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
            cur += read::up(in_len[s], 256) + 8 * (rng() % 3);
        }
        const uint64_t misfit = rng() % 4 == 0 ? rng() % nstreams : nstreams;  // one stream whose chunk_len does not fit
        if (misfit < nstreams) chunk_len[misfit] += 1024;
        std::vector<uint32_t> req_stream(nreq);
        std::vector<uint64_t> start(nreq), len(nreq), off(nreq), clen(nreq), clen2(nreq), clen3(nreq);
        for (uint64_t r = 0; r < nreq; ++r) {
            const uint32_t s = (uint32_t)(rng() % nstreams);
            const uint64_t C = chunk_len[s], n_obj = 4 * C - padding[s];
            req_stream[r] = s;
            switch (rng() % 6) {
                case 0: start[r] = 0; len[r] = n_obj + rng() % 3; break;               // the whole object
                case 1: start[r] = n_obj + rng() % 5000; len[r] = 1 + rng() % 100; break;  // in or past the padding
                case 2: start[r] = rng() % n_obj; len[r] = 0; break;
                case 3: start[r] = C * (1 + rng() % 3) - 5; len[r] = 10; break;         // over a primary boundary
                default: start[r] = rng() % n_obj; len[r] = 1 + rng() % (rng() % 2 ? 64 : 3 * C); break;
            }
        }
        uint64_t total = 0, nseg = 0;
        EXPECT(read::layout(chunk_len.data(), padding.data(), nstreams, req_stream.data(), start.data(), len.data(), nreq,
                            16, off.data(), clen.data(), &total, &nseg) == CHIP_OK);
        const uint64_t need = vread::scratch_len(nreq, nseg);
        EXPECT(need % 16 == 0 && need >= read::scratch_len(nreq, nseg));
        EXPECT(vread::scratch_len(nreq + 1, nseg) >= need && vread::scratch_len(nreq, nseg + 1) >= need);
        vread::Plan p;
        const uint32_t flags = round % 2 ? CHIPV_STRICT : 0u;
        EXPECT(vread::plan_vread(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                                 req_stream.data(), start.data(), len.data(), nreq, OUT, off.data(), clen2.data(), true,
                                 flags, SCR, need, &p) == CHIP_OK);
        // the same plan as a ranged read's: the table, the segments, the totals
        read::Plan q;
        EXPECT(read::plan_read(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                               req_stream.data(), start.data(), len.data(), nreq, OUT, off.data(), clen3.data(), true, SCR,
                               need, &q) == CHIP_OK);
        EXPECT(clen2 == clen3 && p.rd.ka.table == q.ka.table && p.rd.nseg == q.nseg && p.rd.total_blocks == q.total_blocks);
        EXPECT(p.rd.prim_chunks == q.prim_chunks && p.rd.prim_parents == q.prim_parents && p.rd.fb_parents == q.fb_parents);
        const uint64_t ns = p.rd.nseg;
        EXPECT(ns <= nseg && p.lay.total <= need && p.lay.total == vread::scratch_len(nreq, ns));
        EXPECT(p.lay.rd.total == q.lay.total && p.lay.rd.rstat == q.lay.rstat && p.lay.rd.served == q.lay.served);
        // the regions: the ranged read's own (one block up to its total), then the two words per segment;
        // the zeroed range covers exactly rstat, served and the new words, and nothing of the uploaded table
        expect_disjoint({{0, p.lay.rd.table_end},
                         {p.lay.rd.rstat, p.lay.rd.rstat + 32 * ns},
                         {p.lay.rd.served, p.lay.rd.served + ns * sizeof(read::Served)},
                         {p.lay.path, p.lay.path + 4 * ns},
                         {p.lay.contra, p.lay.contra + 4 * ns}},
                        p.lay.total);
        EXPECT(p.lay.path >= p.lay.rd.total && p.lay.path % 16 == 0 && p.lay.contra % 16 == 0);
        EXPECT(p.lay.zero_from() == p.lay.rd.rstat && p.lay.zero_from() >= p.rd.ka.table.size());
        EXPECT(p.lay.zero_from() + p.lay.zero_len() == p.lay.total);
        if (ns) {
            vread::Plan r;
            EXPECT(vread::plan_vread(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                                     req_stream.data(), start.data(), len.data(), nreq, OUT, off.data(), clen2.data(),
                                     true, flags, SCR, p.lay.total - 1, &r) == CHIP_ERR_INVALID_ARG);
        }
        // the shift case: stream and content offsets moved by D, and the two bases moved by D
        for (const uint64_t D : plan_shift::SHIFTS) {
            const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D), off_far = plan_shift::moved(off, D);
            std::vector<uint64_t> len_a(nreq), len_b(nreq);
            vread::Plan by_off, by_base;
            EXPECT(vread::plan_vread(IN, in_far.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                                     req_stream.data(), start.data(), len.data(), nreq, OUT, off_far.data(), len_a.data(),
                                     true, flags, SCR, need, &by_off) == CHIP_OK);
            EXPECT(vread::plan_vread(IN + D, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                                     req_stream.data(), start.data(), len.data(), nreq, OUT + D, off.data(), len_b.data(),
                                     true, flags, SCR, need, &by_base) == CHIP_OK);
            EXPECT(len_a == clen2 && len_b == clen2 && by_off.rd.ka.table == by_base.rd.ka.table);
            EXPECT(by_off.rd.nseg == ns && by_off.vouch_items == p.vouch_items && by_off.lay.total == p.lay.total);
            EXPECT(by_off.rd.total_blocks == p.rd.total_blocks && by_off.rd.fb_parents == p.rd.fb_parents);
            EXPECT(plan_shift::shifted_words(p.rd.ka.table, by_off.rd.ka.table, D) == (long)(3 * ns));
            for (uint64_t k = 0; k < ns; ++k) {
                EXPECT(by_off.rd.segs()[k].src == p.rd.segs()[k].src + D && by_off.rd.segs()[k].dst == p.rd.segs()[k].dst + D);
                EXPECT(by_off.rd.ka.reqs()[k].src == p.rd.ka.reqs()[k].src + D);
            }
        }
        // vouch items: segment g's are its window's chunks, and every item maps back to (segment, chunk) once
        const uint64_t *pre = p.rd.ka.chunks();
        EXPECT(p.vouch_items == pre[ns] && pre[0] == 0);
        std::map<std::pair<uint64_t, uint64_t>, int> seen;
        for (uint64_t g = 0; g < ns; ++g) {
            const read::Seg &sg = p.rd.segs()[g];
            const uint64_t w0 = sg.c0 / 1024, w1 = (sg.c1 + 1023ull) / 1024;
            EXPECT(pre[g + 1] - pre[g] == w1 - w0 && w1 > w0);
        }
        const uint64_t stride = p.vouch_items > 20000 ? 1 + rng() % 7 : 1;  // large windows: a sample, both ends included
        std::vector<uint64_t> items;
        for (uint64_t i = 0; i < p.vouch_items; i += stride) items.push_back(i);
        if (!items.empty() && items.back() + 1 != p.vouch_items) items.push_back(p.vouch_items - 1);
        for (const uint64_t i : items) {
            const uint32_t g = audit::prefix_find(pre, (uint32_t)ns, i);
            EXPECT(g < ns && pre[g] <= i && i < pre[g + 1]);
            const read::Seg &sg = p.rd.segs()[g];
            const audit::Req &a = p.rd.ka.reqs()[g];
            const uint64_t c = a.first + (i - pre[g]);  // as the kernel finds it
            EXPECT(c / sg.spc == sg.p && a.N == 8ull * sg.spc);
            const uint64_t u = c % sg.spc;
            EXPECT(u >= sg.c0 / 1024 && u < (sg.c1 + 1023ull) / 1024 && c < a.last);
            for (uint64_t shard = 0; shard < 8; ++shard) EXPECT(shard * sg.spc + u < a.N);  // the shares' chunks exist
            const int times = ++seen[std::make_pair((uint64_t)g, u)];
            EXPECT(times == 1);
            ++items_seen;
        }
        if (stride == 1) EXPECT(seen.size() == p.vouch_items);
    }
    EXPECT(items_seen > 1000);
    // call-level refusals, in the header's order
    {
        const uint64_t len2[2] = {audit::bao_len(8192), audit::bao_len(8192 * 5)}, off2[2] = {56, 65536 + 8};
        const uint32_t cl[2] = {1024, 5120}, pad[2] = {1, 2}, rs[3] = {0, 1, 1};
        const uint64_t st[3] = {0, 5000, 100}, ln[3] = {100, 9000, 0}, co[3] = {0, 112, 9120};
        uint64_t out[3];
        const uint64_t need = vread::scratch_len(3, 4);
        auto call = [&](uintptr_t in, const uint64_t *il, uintptr_t hash, bool results, uint32_t flags, const uint64_t *o,
                        uintptr_t scr, uint64_t sl, uint64_t nreq = 3) {
            vread::Plan p;
            return vread::plan_vread(in, off2, il, hash, pad, cl, 2, rs, st, ln, nreq, OUT, o, out, results, flags, scr, sl,
                                     &p);
        };
        EXPECT(call(IN, len2, HASH, true, 0, co, SCR, need) == CHIP_OK);
        EXPECT(call(IN, len2, HASH, true, CHIPV_STRICT, co, SCR, need) == CHIP_OK);
        EXPECT(out[0] == 100 && out[1] == 9000 && out[2] == 0);
        EXPECT(call(0, len2, HASH, true, 0, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, len2, HASH, false, 0, co, SCR, need) == CHIP_ERR_INVALID_ARG);  // a NULL result array
        EXPECT(call(IN, len2, HASH, true, 2, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, len2, HASH, true, CHIPV_STRICT | 0x80000000u, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, len2, HASH, true, 0, co, SCR + 8, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, len2, HASH, true, 0, co, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, len2, HASH, true, 0, co, SCR, read::scratch_len(3, 4)) == CHIP_ERR_INVALID_ARG);
        const uint64_t gap[2] = {len2[0] + 8, len2[1]};
        EXPECT(call(IN, gap, HASH, true, 0, co, SCR, need) == CHIP_ERR_BAO_TRUNCATED);
        EXPECT(call(IN, gap, 0, true, 0, co, SCR, need) == CHIP_ERR_BAO_TRUNCATED);
        EXPECT(call(IN, gap, HASH, true, 0, co, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, gap, HASH, true, 4, co, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, len2, 0, true, 0, co, SCR, need) == CHIP_ERR_HASH_DECODE);
        EXPECT(call(IN, len2, 0, true, 0, co, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(0, nullptr, 0, false, 0xFFu, nullptr, 0, 0, 0) == CHIP_OK);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
