// qread_plan_check.cpp — the planning of the device-planned ranged reads
// (carbonado_amd/csrc/qread_device.hpp, the text qread_kernels.hip runs one
// lane per request, compiled here as host code, and qread_plan.hpp, the host's
// O(1) share) driven stand-alone, for a build with -fsanitize=address,undefined
// (tests/test_qread_cpu.py).  No device: the addresses are made-up integers.
//
//  * seeded request sets over streams of C = 1024, 2048, 4096 and 65536, with
//    and without padding, and one whose chunk_len does not fit: every request's
//    status, content length and non-empty segments (read::Seg and the
//    audit::Req slice) equal read::plan_read's, record for record, and the four
//    prefix arrays equal its own with the empty slots removed;
//  * the scan, restated serially, equals audit::finish;
//  * every grid bound is at least the true total: exhaustively for N <= 256,
//    w <= 8 at every window position, and in every seeded call;
//  * S is never smaller than a request's segment count.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/qread_plan.hpp"
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

// exclusive scan in place of n + 1 entries, the last one's count taken as 0:
// what the three scan launches leave
static void scan_serial(std::vector<uint64_t> &a) {
    uint64_t run = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        const uint64_t x = i + 1 < a.size() ? a[i] : 0;
        a[i] = run;
        run += x;
    }
}

static void check_bounds_exhaustive() {
    for (uint64_t N = 1; N <= 256; ++N)
        for (uint64_t w = 1; w <= 8 && w <= N; ++w) {
            const uint64_t bound = qread::slice_parents_bound(N, w);
            for (uint64_t f = 0; f + w <= N; ++f) EXPECT(audit::sel_parents(N, f, f + w) <= bound);
            // monotone in both, so the bound of (max_chunks, W) covers every smaller tree and window
            EXPECT(qread::slice_parents_bound(N + 1, w) >= bound && qread::slice_parents_bound(N, w + 1) >= bound);
        }
    for (uint64_t N : {1000ull, 4096ull, 65537ull, 1ull << 20})
        for (uint64_t w = 1; w <= 8; ++w)
            for (uint64_t f : {(uint64_t)0, (uint64_t)1, N / 2 - 1, N / 2, N - w})
                EXPECT(audit::sel_parents(N, f, f + w) <= qread::slice_parents_bound(N, w));
    // blocks of the read kernel: every length to 3 blocks and every address residue
    for (uint64_t l = 1; l <= 3 * read::BLOCK; ++l)
        for (uint64_t a = 0; a < 16; ++a) {
            const uint64_t dst = 0x1000 + a;
            const uint64_t blocks = (read::units_of(dst, dst + l) * read::UNIT + read::BLOCK - 1) / read::BLOCK;
            EXPECT(blocks <= (l + 2 * (read::UNIT - 1) + read::BLOCK - 1) / read::BLOCK);
        }
    // chunks a range touches
    for (uint64_t l = 1; l <= 5000; ++l)
        for (uint64_t s : {0ull, 1ull, 1023ull, 1024ull, 1500ull})
            EXPECT((s + l - 1) / 1024 - s / 1024 + 1 <= qread::window_bound(l));
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    check_bounds_exhaustive();
    const uintptr_t IN = 0x10000000, OUT = 0x4000000000, HASH = 0x70000000, SCR = 0x7800000000, TAB = 0x7900000000;
    const uint32_t shard[] = {1024, 2048, 4096, 65536};
    uint64_t seen_long = 0;  // requests whose clipped content is above the capacity
    for (int round = 0; round < 120; ++round) {
        const uint64_t nstreams = 5 + rng() % 6, nreq = 1 + rng() % 70;
        std::vector<uint64_t> in_off(nstreams), in_len(nstreams);
        std::vector<uint32_t> chunk_len(nstreams), padding(nstreams);
        uint64_t cur = 56;
        for (uint64_t s = 0; s < nstreams; ++s) {
            const uint32_t C = s < 4 ? shard[s] : shard[rng() % 4];
            chunk_len[s] = C;
            padding[s] = s % 2 ? 0 : (uint32_t)(rng() % (4 * C));  // even streams padded, stream 0 perhaps down to 1 byte
            in_off[s] = cur;
            in_len[s] = audit::bao_len(8ull * C);
            cur += audit::up(in_len[s], 8) + 8 * (rng() % 4);
        }
        chunk_len[4] = chunk_len[4] == 1024 ? 2048 : 1024;  // a chunk_len that does not fit its stream's length
        if (round % 7 == 3) padding[nstreams - 1] = 4 * chunk_len[nstreams - 1] + 1;  // and a padding that does not
        const uint64_t max_len = round % 2 ? 5000 : 4096, stride = audit::up(max_len, 16) + 16 * (rng() % 3);

        chipq_table_info info;
        std::vector<uint8_t> table;
        EXPECT(qread::plan_table(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams, TAB,
                                 qread::table_len(nstreams), &info, &table) == CHIP_OK);
        EXPECT(info.nstreams == nstreams && info.min_shard == 1024 && info.max_chunks >= 8 && info.reserved == 0);
        const qread::StreamRec *recs = reinterpret_cast<const qread::StreamRec *>(table.data());
        EXPECT(recs[4].C == 0);
        // the shift case: every stream offset moved by D, and the base moved by D: the same table, each record's
        // stream address D higher, the same info; and a call whose content base and stride lie past 2^32
        for (const uint64_t D : plan_shift::SHIFTS) {
            const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D);
            chipq_table_info info2, info3;
            std::vector<uint8_t> by_off, by_base;
            EXPECT(qread::plan_table(IN, in_far.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams, TAB,
                                     qread::table_len(nstreams), &info2, &by_off) == CHIP_OK);
            EXPECT(qread::plan_table(IN + D, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                                     TAB, qread::table_len(nstreams), &info3, &by_base) == CHIP_OK);
            EXPECT(by_off == by_base && !std::memcmp(&info2, &info, sizeof info) && !std::memcmp(&info3, &info, sizeof info));
            EXPECT(plan_shift::shifted_words(table, by_off, D) == (long)nstreams);
            const qread::StreamRec *far = reinterpret_cast<const qread::StreamRec *>(by_off.data());
            for (uint64_t k = 0; k < nstreams; ++k) EXPECT(far[k].src == recs[k].src + D && far[k].hash == recs[k].hash);
            qread::Geometry g1, g2;
            qread::ScratchLayout l1, l2;
            const uint64_t need = qread::scratch_len(&info, nreq, max_len, true);
            EXPECT(qread::plan_call(TAB, &info, true, nreq, max_len, OUT, stride, true, true, 0, SCR, need, &g1, &l1) == CHIP_OK);
            EXPECT(qread::plan_call(TAB, &info, true, nreq, max_len, OUT + D, D + 256, true, true, 0, SCR, need, &g2, &l2) ==
                   CHIP_OK);
            EXPECT(g1.ok && g2.ok && g1.S == g2.S && g1.nslot == g2.nslot && g1.blocks == g2.blocks && g1.parents == g2.parents);
            EXPECT(l1.total == l2.total && l1.total <= need && l1.segs == l2.segs && l1.contra == l2.contra);
        }

        std::vector<uint32_t> rs(nreq);
        std::vector<uint64_t> start(nreq), len(nreq), coff(nreq);
        for (uint64_t r = 0; r < nreq; ++r) {
            rs[r] = (uint32_t)(rng() % nstreams);
            const uint64_t n_obj = padding[rs[r]] > 4ull * chunk_len[rs[r]] ? 100 : 4ull * chunk_len[rs[r]] - padding[rs[r]];
            const uint64_t C = chunk_len[rs[r]];
            switch (rng() % 8) {
            case 0: start[r] = rng() % (n_obj + 10); len[r] = rng() % 64; break;                // inside a chunk, or empty
            case 1: start[r] = C * (1 + rng() % 3) - 1 - rng() % 100; len[r] = 200; break;      // across a shard boundary
            case 2:  // the whole capacity, and where the slot has room, more: the device refuses that request alone
                start[r] = rng() % (n_obj + 1);
                len[r] = max_len + (round % 4 == 1 && rng() % 2 ? rng() % (stride - max_len + 1) : 0);  // (3 rounds in 4 keep to it)
                break;
            case 3: start[r] = n_obj - audit::umin(n_obj, rng() % 3000); len[r] = 1ull << 40; break;  // clipped at the end
            case 4: start[r] = rng() % 2000; len[r] = 1 + rng() % max_len; break;
            case 5: start[r] = 1024 * (rng() % 4) + rng() % 16; len[r] = max_len - rng() % 16; break;
            case 6: start[r] = n_obj + rng() % 5; len[r] = 7; break;                            // start at or past the end
            default: start[r] = rng() % (n_obj + 1); len[r] = rng() % (max_len + 1); break;
            }
            coff[r] = r * stride;
        }
        // the host plan refuses a whole call for what the device refuses per request: keep those out of its set
        std::vector<uint64_t> clen(nreq);
        read::Plan hp;
        const int st = read::plan_read(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), nstreams,
                                       rs.data(), start.data(), len.data(), nreq, OUT, coff.data(), clen.data(), true,
                                       SCR, ~0ull, &hp);
        EXPECT(st == CHIP_OK);
        for (uint64_t r = 0; r < nreq; ++r) seen_long += clen[r] > max_len;

        const qread::Geometry g(info, nreq, max_len);
        EXPECT(g.ok && g.S == 4 && g.nslot == 4 * nreq);
        const qread::ScratchLayout lay(g, nreq, true);
        EXPECT(lay.total % 16 == 0 && qread::scratch_len(&info, nreq, max_len, true) == lay.total);
        EXPECT(qread::scratch_len(&info, nreq, max_len, false) < lay.total);
        const qread::Shape sh{info.nstreams, info.max_chunks, info.min_shard, max_len, g.S};
        std::vector<read::Req> reqs(nreq);
        std::vector<read::Seg> segs(g.nslot);
        std::vector<audit::Req> slices(g.nslot);
        std::vector<uint64_t> pre[4], qlen(nreq);
        for (auto &a : pre) a.assign(g.nslot + 1, ~0ull);
        const qread::Tables t{reqs.data(), segs.data(), slices.data(), pre[0].data(), pre[1].data(), pre[2].data(),
                              pre[3].data(), qlen.data()};
        for (uint64_t r = 0; r < nreq; ++r)
            qread::plan_request(recs, sh, (uint32_t)r, rs[r], start[r], len[r], OUT + r * stride, t);
        for (auto &a : pre) scan_serial(a);

        // record for record against the host plan
        uint64_t g2 = 0;
        std::vector<uint64_t> packed[4];
        for (uint64_t r = 0; r < nreq; ++r) {
            const read::Req &h = hp.reqs()[r], &q = reqs[r];
            const bool too_long = clen[r] > max_len;
            EXPECT(q.seg0 == r * g.S && q.pad_ == 0);
            if (too_long) {  // what the host-planned call has no word for
                EXPECT(q.status == CHIP_ERR_INVALID_ARG && q.nseg == 0 && qlen[r] == 0);
                g2 += h.nseg;
                continue;
            }
            EXPECT(q.status == h.status && q.nseg == h.nseg && qlen[r] == clen[r] && h.nseg <= g.S);
            for (uint32_t k = 0; k < g.S; ++k) {
                const uint64_t slot = q.seg0 + k;
                if (k >= q.nseg) {
                    for (auto &a : pre) EXPECT(a[slot + 1] == a[slot]);  // no items
                    continue;
                }
                const read::Seg &a = hp.segs()[h.seg0 + k], &b = segs[slot];
                EXPECT(a.src == b.src && a.dst == b.dst && a.N == b.N && a.spc == b.spc && a.c0 == b.c0 && a.c1 == b.c1 &&
                       a.p == b.p && a.req == b.req);
                EXPECT(std::memcmp(&hp.ka.reqs()[h.seg0 + k], &slices[slot], sizeof(audit::Req)) == 0);
                const uint64_t hg = h.seg0 + k;
                EXPECT(pre[0][slot + 1] - pre[0][slot] == hp.ka.parents()[hg + 1] - hp.ka.parents()[hg]);
                EXPECT(pre[1][slot + 1] - pre[1][slot] == hp.ka.chunks()[hg + 1] - hp.ka.chunks()[hg]);
                EXPECT(pre[2][slot + 1] - pre[2][slot] == hp.fpar()[hg + 1] - hp.fpar()[hg]);
                EXPECT(pre[3][slot + 1] - pre[3][slot] == hp.blocks()[hg + 1] - hp.blocks()[hg]);
                for (int a4 = 0; a4 < 4; ++a4) packed[a4].push_back(pre[a4][slot]);
            }
            g2 += h.nseg;
        }
        EXPECT(g2 == hp.nseg);
        for (int a4 = 0; a4 < 4; ++a4) {
            EXPECT(pre[a4][0] == 0);
            packed[a4].push_back(pre[a4][g.nslot]);
        }
        bool any_long = false;
        for (uint64_t r = 0; r < nreq; ++r) any_long |= clen[r] > max_len;
        if (!any_long) {  // the prefix arrays with the empty slots removed are the host plan's, audit::finish's among them
            EXPECT(packed[0].size() == hp.nseg + 1);
            for (uint64_t i = 0; i <= hp.nseg && packed[0].size() == hp.nseg + 1; ++i) {
                EXPECT(packed[0][i] == hp.ka.parents()[i] && packed[1][i] == hp.ka.chunks()[i]);
                EXPECT(packed[2][i] == hp.fpar()[i] && packed[3][i] == hp.blocks()[i]);
            }
            EXPECT(pre[0][g.nslot] == hp.prim_parents && pre[1][g.nslot] == hp.prim_chunks);
            EXPECT(pre[2][g.nslot] == hp.fb_parents && pre[3][g.nslot] == hp.total_blocks);
        }
        // the grids are bounds
        EXPECT(pre[0][g.nslot] <= g.parents && pre[1][g.nslot] <= g.chunks && pre[2][g.nslot] <= g.fb_parents);
        EXPECT(pre[3][g.nslot] <= g.blocks);  // (fallback chunk items are 7 x the chunk items on both sides)
        EXPECT(g.scan_blocks * qread::SCAN_TILE >= g.nslot + 1);

        // requests the device refuses
        const struct { uint32_t s; uint64_t start, len; } bad[] = {
            {(uint32_t)nstreams, 0, 1}, {0, (1ull << 53) + 1, 1}, {0, 0, (1ull << 53) + 1}, {1, 0, max_len + 1}};
        for (const auto &b : bad) {
            qread::plan_request(recs, sh, 0, b.s, b.start, b.len, OUT, t);
            EXPECT(reqs[0].status == CHIP_ERR_INVALID_ARG && reqs[0].nseg == 0 && qlen[0] == 0);
            for (auto &a : pre) EXPECT(a[0] == 0 && a[1] == 0 && a[2] == 0 && a[3] == 0);
        }
        qread::plan_request(recs, sh, 0, 4, 0, 10, OUT, t);  // the stream that does not fit
        EXPECT(reqs[0].status == CHIP_ERR_ZFEC && reqs[0].nseg == 0 && qlen[0] == 0);
        qread::Shape lie = sh;
        lie.max_chunks = info.max_chunks - 1;  // an info that is not the table's
        for (uint32_t s = 0; s < nstreams; ++s) {
            qread::plan_request(recs, lie, 0, s, 0, 10, OUT, t);
            EXPECT((reqs[0].status == CHIP_ERR_INVALID_ARG) == (recs[s].N == info.max_chunks));
        }
        lie = sh;
        lie.min_shard = 2048;
        qread::plan_request(recs, lie, 0, 0, 0, 10, OUT, t);
        EXPECT(reqs[0].status == CHIP_ERR_INVALID_ARG);
    }

    std::printf("%llu requests above the capacity\n", (unsigned long long)seen_long);
    EXPECT(seen_long > 5);

    // segment slots: S is the most segments a range of max_len bytes can have
    for (uint64_t C : {1024ull, 2048ull, 4096ull, 65536ull})
        for (uint64_t max_len : {1ull, 2ull, 1024ull, 1025ull, 1026ull, 2049ull, 4096ull, 5000ull, 70000ull, 1ull << 40}) {
            const uint32_t S = qread::slots_of(C, max_len);
            EXPECT(S >= 1 && S <= 4);
            uint32_t most = 0;
            for (uint64_t start : {(uint64_t)0, (uint64_t)1, C - 1, C, 2 * C - 1, 3 * C - 1, 4 * C - 1}) {
                const read::Range rg = read::range_of(C, 0, start, max_len);
                most = std::max(most, rg.nseg);
                EXPECT(rg.nseg <= S);
            }
            EXPECT(most == S);
        }
    EXPECT(qread::slots_of(0, 4096) == 1);

    // the host checks of a call, in the header's order
    {
        chipq_table_info info{3, 512, 1024, 0};
        qread::Geometry g;
        qread::ScratchLayout lay;
        const uint64_t need = qread::scratch_len(&info, 10, 4096, true);
        auto call = [&](uintptr_t tab, const chipq_table_info *i, bool reqs, uint64_t nreq, uint64_t max_len, uintptr_t out,
                        uint64_t stride, bool res, uint32_t flags, uintptr_t scr, uint64_t sl) {
            return qread::plan_call(tab, i, reqs, nreq, max_len, out, stride, res, true, flags, scr, sl, &g, &lay);
        };
        EXPECT(need && need % 16 == 0);
        EXPECT(call(0, nullptr, false, 0, 0, 0, 0, false, 9, 0, 0) == CHIP_OK);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT, 4096, true, 1, SCR, need) == CHIP_OK);
        EXPECT(call(0, &info, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, nullptr, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, false, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT, 4096, false, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 1ull << 31, 4096, OUT, 4096, true, 0, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 0, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, (1ull << 53) + 1, OUT, 1ull << 54, true, 0, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT, 4088, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4097, OUT, 4096, true, 0, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT + 8, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT, 1ull << 62, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT, 4096, true, 2, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 1 << 30, 1ull << 20, OUT, 1ull << 20, true, 0, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(TAB, &info, true, 10, 4096, OUT, 4096, true, 0, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
        EXPECT(qread::scratch_len(&info, 1 << 30, 1ull << 20, true) == 0 && qread::scratch_len(nullptr, 1, 1, true) == 0);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
