// audit_plan_check.cpp — the host logic of the slice audits
// (carbonado_amd/csrc/audit_plan.hpp: layout, argument checks, request table
// and prefix arrays) and the item-to-node arithmetic the kernels share with it
// (audit_nodes.hpp), driven stand-alone for a build with
// -fsanitize=address,undefined (tests/test_audit_cpu.py).  No device: the
// addresses are made-up integers, nothing is dereferenced.
//
//   audit_plan_check nodes n index count [n index count ...]
//       every work item of each request, enumerated as the kernels do it:
//         req <n> <index> <count> <N> <first> <last> <parents> <proof_len> <content_len>
//         node <P|C> <level> <leftmost chunk> <stream offset> <bytes> <proof offset> <slot in stream> <slot in proof>
//       (slot: where the 32 bytes the node is compared with sit; -1 = the root)
//   audit_plan_check plan <seed>
//       seeded mixes of requests through plan_extract / plan_verify and the
//       layout; prints "<k> failures"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../carbonado_amd/csrc/audit_plan.hpp"
#include "plan_shift.hpp"

using namespace chip::audit;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

struct Node {
    bool parent;
    int level;
    uint64_t s, soff, size, poff;
    int64_t slot_s, slot_p;
};

// the work items of one request, in item order: parents, then chunks
static std::vector<Node> items(uint64_t n, const Sel &sel) {
    std::vector<Node> out;
    const uint64_t N = sel.N, f = sel.first, l = sel.last;
    for (uint64_t k = 0; k < sel.parents; ++k) {
        uint64_t s = 0;
        const int lv = parent_item(N, f, l, k, &s);
        const bool root = is_root(s, lv, N);
        out.push_back({true, lv, s, node_off<false>(s, lv, N, f, l), 64, node_off<true>(s, lv, N, f, l),
                       root ? -1 : (int64_t)slot_off<false>(s, lv, N, f, l),
                       root ? -1 : (int64_t)slot_off<true>(s, lv, N, f, l)});
    }
    for (uint64_t c = f; c < l; ++c)
        out.push_back({false, 0, c, node_off<false>(c, 0, N, f, l), chunk_len(c, n), node_off<true>(c, 0, N, f, l),
                       N == 1 ? -1 : (int64_t)slot_off<false>(c, 0, N, f, l),
                       N == 1 ? -1 : (int64_t)slot_off<true>(c, 0, N, f, l)});
    return out;
}

static int print_nodes(int argc, char **argv) {
    for (int a = 2; a + 2 < argc; a += 3) {
        const uint64_t n = std::strtoull(argv[a], nullptr, 0), index = std::strtoull(argv[a + 1], nullptr, 0),
                       count = std::strtoull(argv[a + 2], nullptr, 0);
        const Sel sel = select(n, index, count);
        std::printf("req %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                    " %" PRIu64 "\n", n, index, count, sel.N, sel.first, sel.last, sel.parents, sel.proof_len, sel.olen);
        for (const Node &nd : items(n, sel))
            std::printf("node %c %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 "\n",
                        nd.parent ? 'P' : 'C', nd.level, nd.s, nd.soff, nd.size, nd.poff, nd.slot_s, nd.slot_p);
    }
    return 0;
}

// The items of a request tile its proof exactly, in strictly increasing stream
// order, every slot lies inside a selected parent, and the full-range request
// reproduces the stream.
static void check_request(uint64_t n, uint64_t index, uint64_t count) {
    const Sel sel = select(n, index, count);
    EXPECT(sel.first < sel.last && sel.last <= sel.N);
    std::vector<Node> nd = items(n, sel);
    EXPECT(nd.size() == sel.parents + (sel.last - sel.first));
    std::sort(nd.begin(), nd.end(), [](const Node &a, const Node &b) { return a.poff < b.poff; });
    uint64_t at = 8, prev = 0;
    for (const Node &x : nd) {
        EXPECT(x.poff == at);
        EXPECT(x.soff >= 8 && x.soff > prev && x.soff + x.size <= bao_len(n));
        prev = x.soff;
        at += x.size;
        if (x.slot_p >= 0) {  // the slot is a half of a selected parent, at the same place in stream and proof
            bool found = false;
            for (const Node &y : nd)
                if (y.parent && (uint64_t)x.slot_p >= y.poff && (uint64_t)x.slot_p < y.poff + 64) {
                    found = (x.slot_p - (int64_t)y.poff) % 32 == 0 &&
                            x.slot_s - (int64_t)y.soff == x.slot_p - (int64_t)y.poff;
                    break;
                }
            EXPECT(found);
        }
    }
    EXPECT(at == sel.proof_len);
    if (sel.first == 0 && sel.last == sel.N) {
        EXPECT(sel.proof_len == bao_len(n));
        for (const Node &x : nd) EXPECT(x.poff == x.soff);
    }
    const uint64_t start = index * 1024;
    EXPECT(sel.olen == (start < n ? umin(n, start + count * 1024) - start : 0));
}

// ranges_overlap against every pair compared: seeded sets of up to 12 ranges that
// tile a line with gaps (so neighbours touch or stand apart), some of them empty
// and lying anywhere, in ascending or shuffled order, with or without one range
// stretched into its successor, which is also placed at the last pair
static bool overlap_plain(const std::vector<uint64_t> &off, const std::vector<uint64_t> &len) {
    for (size_t a = 0; a < off.size(); ++a)
        for (size_t b = a + 1; b < off.size(); ++b)
            if (len[a] && len[b] && off[a] < off[b] + len[b] && off[b] < off[a] + len[a]) return true;
    return false;
}

static void check_overlaps(std::mt19937_64 &rng) {
    int seen[2][2] = {{0, 0}, {0, 0}};  // [shuffled][overlapping]
    for (int round = 0; round < 400; ++round) {
        const size_t count = rng() % 13;
        std::vector<uint64_t> off(count), len(count);
        uint64_t cur = rng() % 64;
        for (size_t r = 0; r < count; ++r) {
            off[r] = cur;
            len[r] = rng() % 4 == 0 ? 0 : 1 + rng() % 100;  // zero-length members
            cur += len[r] + (rng() % 2 ? 0 : rng() % 50);   // touching, or a gap
            if (!len[r] && rng() % 2) off[r] = rng() % (cur + 1);  // an empty range overlaps nothing, wherever it lies
        }
        std::vector<size_t> full;
        for (size_t r = 0; r < count; ++r)
            if (len[r]) full.push_back(r);
        const int kind = round % 3;  // 0: disjoint, 1: one overlap somewhere, 2: one overlap at the last pair
        if (kind && full.size() >= 2) {
            const size_t at = kind == 2 ? full.size() - 2 : rng() % (full.size() - 1);
            len[full[at]] = off[full[at + 1]] - off[full[at]] + 1 + rng() % 3;
        }
        const bool shuffled = round % 2;
        if (shuffled)
            for (size_t r = count; r > 1; --r) {
                const size_t j = rng() % r;
                std::swap(off[r - 1], off[j]);
                std::swap(len[r - 1], len[j]);
            }
        const bool want = overlap_plain(off, len);
        EXPECT(want == (kind && full.size() >= 2));
        EXPECT(ranges_overlap(off.data(), len.data(), count) == want);
        ++seen[shuffled][want];
    }
    EXPECT(seen[0][0] > 20 && seen[0][1] > 20 && seen[1][0] > 20 && seen[1][1] > 20);
    EXPECT(!ranges_overlap(nullptr, nullptr, 0));
}

static int plan_mode(unsigned seed) {
    std::mt19937_64 rng(seed), own(seed ^ 0x0FF5E7u);  // (the mixes below keep their sequence)
    check_overlaps(own);
    const uintptr_t STREAMS = 0x10000000, PROOFS = 0x400000000, CONTENT = 0x800000000, HASH = 0x70000000;
    EXPECT(select(0, MAX_SLICE, MAX_SLICE).olen == 0);  // the largest request wraps nowhere
    EXPECT(select(MAX_CONTENT, MAX_SLICE, MAX_SLICE).last == chunks(MAX_CONTENT));
    for (int round = 0; round < 60; ++round) {
        const uint64_t nstreams = 1 + rng() % 12, nreq = rng() % 60;
        std::vector<uint64_t> n(nstreams), in_off(nstreams), in_len(nstreams);
        uint64_t cur = 8 * (rng() % 32);
        for (uint64_t s = 0; s < nstreams; ++s) {
            const int kind = (int)(rng() % 4);
            n[s] = kind == 0 ? rng() % 1100 : kind == 1 ? rng() % 70000 : kind == 2 ? rng() % (3u << 20) : 1024 * (rng() % 300);
            in_off[s] = cur;
            in_len[s] = bao_len(n[s]);
            uint64_t back = 0;
            EXPECT(bao_content(in_len[s], &back) && back == n[s]);
            cur += up(in_len[s], 8) + 8 * (rng() % 8);
        }
        std::vector<uint32_t> rs(nreq);
        std::vector<uint64_t> index(nreq), count(nreq), cl(nreq);
        for (uint64_t r = 0; r < nreq; ++r) {
            rs[r] = (uint32_t)(rng() % nstreams);
            const uint64_t N = chunks(n[rs[r]]);
            index[r] = rng() % (N + 3);
            count[r] = rng() % 3 == 0 ? rng() % (N + 2) : rng() % 4;
            cl[r] = n[rs[r]];
            if (round < 20) check_request(cl[r], index[r], count[r]);
        }
        const uint64_t align = 16 * (1 + rng() % 16);
        std::vector<uint64_t> po(nreq), pl(nreq), co(nreq), clo(nreq), clo2(nreq);
        uint64_t pt = 0, ct = 0;
        EXPECT(layout(cl.data(), index.data(), count.data(), nreq, align, po.data(), pl.data(), co.data(), clo.data(),
                      &pt, &ct) == CHIP_OK);
        EXPECT(!ranges_overlap(po.data(), pl.data(), nreq) && !ranges_overlap(co.data(), clo.data(), nreq));
        for (uint64_t r = 0; r < nreq; ++r)
            EXPECT(po[r] % align == 0 && co[r] % align == 0 && po[r] + pl[r] <= pt && co[r] + clo[r] <= ct);
        Plan x, v, w;
        EXPECT(plan_extract(STREAMS, in_off.data(), in_len.data(), nstreams, rs.data(), index.data(), count.data(), nreq,
                            PROOFS, po.data(), pl.data(), &x) == CHIP_OK);
        EXPECT(plan_verify(false, STREAMS, in_off.data(), in_len.data(), nstreams, rs.data(), nullptr, HASH,
                           index.data(), count.data(), nreq, CONTENT, co.data(), clo2.data(), true, &v) == CHIP_OK);
        EXPECT(clo2 == clo);
        EXPECT(plan_verify(true, PROOFS, po.data(), pl.data(), nreq, nullptr, cl.data(), HASH, index.data(),
                           count.data(), nreq, CONTENT, co.data(), clo2.data(), true, &w) == CHIP_OK);
        if (nreq == 0) continue;
        for (Plan *p : {&x, &v, &w}) {  // the invariants the kernels rely on
            EXPECT(p->table.size() + 16 == scratch_len(nstreams, nreq) && p->nreq == nreq);
            EXPECT(p->parents()[0] == 0 && p->chunks()[0] == 0 && p->units()[0] == 0);
            EXPECT(p->parents()[nreq] == p->total_parents && p->chunks()[nreq] == p->total_chunks &&
                   p->units()[nreq] == p->total_units);
            for (uint64_t r = 0; r < nreq; ++r) {
                const Req &q = p->reqs()[r];
                const Sel sel = select(cl[r], index[r], count[r]);
                EXPECT(q.n == cl[r] && q.N == sel.N && q.first == sel.first && q.last == sel.last && q.olen == sel.olen);
                EXPECT(p->parents()[r + 1] - p->parents()[r] == sel.parents);
                EXPECT(p->chunks()[r + 1] - p->chunks()[r] == sel.last - sel.first);
                EXPECT(p->units()[r + 1] - p->units()[r] ==
                       (p == &x ? extract_units(sel.parents, sel.last - sel.first) : (sel.olen + 15) / 16));
                EXPECT(q.src % 8 == 0 && q.dst % (p == &x ? 8 : 16) == 0);
            }
        }
        // the shift case: stream, proof and content offsets moved by D, and the three bases moved by D
        for (const uint64_t D : plan_shift::SHIFTS) {
            const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D), po_far = plan_shift::moved(po, D),
                                        co_far = plan_shift::moved(co, D);
            std::vector<uint64_t> la(nreq), lb(nreq);
            Plan xo, xb, vo, vb, wo, wb;
            EXPECT(plan_extract(STREAMS, in_far.data(), in_len.data(), nstreams, rs.data(), index.data(), count.data(),
                                nreq, PROOFS, po_far.data(), pl.data(), &xo) == CHIP_OK);
            EXPECT(plan_extract(STREAMS + D, in_off.data(), in_len.data(), nstreams, rs.data(), index.data(), count.data(),
                                nreq, PROOFS + D, po.data(), pl.data(), &xb) == CHIP_OK);
            EXPECT(plan_verify(false, STREAMS, in_far.data(), in_len.data(), nstreams, rs.data(), nullptr, HASH,
                               index.data(), count.data(), nreq, CONTENT, co_far.data(), la.data(), true, &vo) == CHIP_OK);
            EXPECT(plan_verify(false, STREAMS + D, in_off.data(), in_len.data(), nstreams, rs.data(), nullptr, HASH,
                               index.data(), count.data(), nreq, CONTENT + D, co.data(), lb.data(), true, &vb) == CHIP_OK);
            EXPECT(la == clo && lb == clo);
            EXPECT(plan_verify(true, PROOFS, po_far.data(), pl.data(), nreq, nullptr, cl.data(), HASH, index.data(),
                               count.data(), nreq, CONTENT, co_far.data(), la.data(), true, &wo) == CHIP_OK);
            EXPECT(plan_verify(true, PROOFS + D, po.data(), pl.data(), nreq, nullptr, cl.data(), HASH, index.data(),
                               count.data(), nreq, CONTENT + D, co.data(), lb.data(), true, &wb) == CHIP_OK);
            EXPECT(la == clo && lb == clo);
            Plan *first[3] = {&x, &v, &w}, *by_off[3] = {&xo, &vo, &wo}, *by_base[3] = {&xb, &vb, &wb};
            for (int k = 0; k < 3; ++k) {
                EXPECT(by_off[k]->table == by_base[k]->table);
                EXPECT(by_off[k]->total_parents == first[k]->total_parents && by_off[k]->total_chunks == first[k]->total_chunks &&
                       by_off[k]->total_units == first[k]->total_units);
                // per request: where it reads and where it writes, D higher; nothing else changed
                EXPECT(plan_shift::shifted_words(first[k]->table, by_off[k]->table, D) == (long)(2 * nreq));
                for (uint64_t r = 0; r < nreq; ++r) {
                    const Req &q = first[k]->reqs()[r], &f = by_off[k]->reqs()[r];
                    EXPECT(f.src == q.src + D && f.dst == q.dst + D && f.hash == q.hash);
                }
            }
            EXPECT(!ranges_overlap(po_far.data(), pl.data(), nreq) && !ranges_overlap(co_far.data(), clo.data(), nreq));
        }
        // one thing wrong at a time
        const uint64_t a = rng() % nreq;
        std::vector<uint64_t> bad = co;
        bad[a] += 8;
        EXPECT(plan_verify(false, STREAMS, in_off.data(), in_len.data(), nstreams, rs.data(), nullptr, HASH,
                           index.data(), count.data(), nreq, CONTENT, bad.data(), clo2.data(), true, &v) ==
               CHIP_ERR_INVALID_ARG);
        bad = po;
        bad[a] += 4;
        EXPECT(plan_extract(STREAMS, in_off.data(), in_len.data(), nstreams, rs.data(), index.data(), count.data(), nreq,
                            PROOFS, bad.data(), pl.data(), &x) == CHIP_ERR_INVALID_ARG);
        bad = pl;
        bad[a] += 64;
        EXPECT(plan_verify(true, PROOFS, po.data(), bad.data(), nreq, nullptr, cl.data(), HASH, index.data(),
                           count.data(), nreq, CONTENT, co.data(), clo2.data(), true, &w) == CHIP_ERR_BAO_TRUNCATED);
        std::vector<uint32_t> brs = rs;
        brs[a] = (uint32_t)nstreams;
        EXPECT(plan_verify(false, STREAMS, in_off.data(), in_len.data(), nstreams, brs.data(), nullptr, HASH,
                           index.data(), count.data(), nreq, CONTENT, co.data(), clo2.data(), true, &v) ==
               CHIP_ERR_INVALID_ARG);
        if (nreq >= 2) {
            const uint64_t b = (a + 1) % nreq;
            bad = po;
            bad[b] = bad[a];  // proofs are never empty
            EXPECT(plan_extract(STREAMS, in_off.data(), in_len.data(), nstreams, rs.data(), index.data(), count.data(),
                                nreq, PROOFS, bad.data(), pl.data(), &x) == CHIP_ERR_INVALID_ARG);
        }
    }
    // every small tree, every request
    for (uint64_t N = 1; N <= 20; ++N)
        for (uint64_t n : {N * 1024, N * 1024 - 1023, N * 1024 - 5})
            for (uint64_t i = 0; i <= N + 1; ++i)
                for (uint64_t c = 0; c <= N + 1; ++c) check_request(n, i, c);
    check_request(0, 0, 0);
    check_request(0, 3, 2);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 5 && !std::strcmp(argv[1], "nodes")) return print_nodes(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "plan"))
        return plan_mode(argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 0) : 1u);
    std::fprintf(stderr, "usage: %s nodes n index count [...] | plan [seed]\n", argv[0]);
    return 2;
}
