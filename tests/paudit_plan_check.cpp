// paudit_plan_check.cpp — the planning of the device-planned slice audits
// (carbonado_amd/csrc/paudit_device.hpp, the text paudit_kernels.hip runs one
// lane per request and its work-item arithmetic, compiled here as host code,
// and paudit_plan.hpp, the host's O(1) share) driven stand-alone, for a build
// with -fsanitize=address,undefined (tests/test_paudit_cpu.py).  No device: the
// addresses are made-up integers.
//
//  * seeded request sets over streams of the GPU tests' sizes, an index past
//    the end, a count of 0 and a count of 2^53 among them: every request's
//    record, parent count, status, content length and proof length equal
//    audit::plan_verify's / audit::plan_extract's, record for record, on the
//    holder's side and the auditor's; what the device refuses is refused;
//  * exhaustively for N <= 256, w <= 8: P is at least the true parent count and
//    chipp_proof_bound at least the true proof length;
//  * the item -> (request, slot) arithmetic covers every true work item of the
//    four item kinds exactly once;
//  * the order of the host checks of the root table and of the three calls.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../carbonado_amd/csrc/paudit_plan.hpp"
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

static const uint64_t SIZES[] = {0, 1, 1023, 1024, 1025, 3072, 5121, 8192, 8193, 13317, 24576, 66561};
constexpr uint64_t NS = sizeof SIZES / sizeof SIZES[0];

static void check_bounds_exhaustive() {
    for (uint64_t N = 1; N <= 256; ++N)
        for (uint64_t w = 1; w <= 8; ++w) {
            const paudit::Geometry g(N, 1, w);
            EXPECT(g.ok && g.W == audit::umin(w, N) && g.P == qread::slice_parents_bound(N, g.W));
            const uint64_t bound = paudit::proof_bound(N, w);
            EXPECT(bound == 8 + 64 * qread::slice_parents_bound(N, w) + 1024 * w && bound >= 8 + 64 * g.P + 1024 * g.W);
            // every selection of w chunks or fewer; both bounds grow with N and w, so they cover every smaller tree
            for (uint64_t f = 0; f < N; ++f)
                for (uint64_t l = f + 1; l <= N && l - f <= w; ++l) {
                    EXPECT(audit::sel_parents(N, f, l) <= g.P);
                    EXPECT(8 + 64 * audit::sel_parents(N, f, l) + 1024 * (l - f) <= bound);
                }
            EXPECT(paudit::Geometry(N + 1, 1, w).P >= g.P && paudit::Geometry(N, 1, w + 1).P >= g.P);
            EXPECT(paudit::proof_bound(N + 1, w) >= bound && paudit::proof_bound(N, w + 1) >= bound);
        }
    EXPECT(paudit::proof_bound(1024, 0) == 0 && paudit::proof_bound(1024, (1ull << 53) + 1) == 0);
    EXPECT(paudit::proof_bound(1024, 1ull << 53) > (1ull << 63));
    EXPECT(paudit::proof_bound(1, 1) == 8 + 1024 && paudit::proof_bound(0, 1) == 8 + 1024);
}

// every true work item of a call, by the kernels' arithmetic, exactly once
static void check_mapping(const std::vector<paudit::Planned> &pl, const paudit::Geometry &g) {
    const uint64_t nreq = pl.size();
    std::map<std::tuple<int, uint64_t, uint64_t, uint64_t>, int> seen;  // kind, request, slot, unit
    for (uint64_t i = 0; i < g.parents; ++i) {  // the parent check
        const paudit::Item it = paudit::item_of(i, nreq, 1);
        EXPECT(it.r < nreq && it.slot < g.P && it.unit == 0);
        if (it.slot < pl[it.r].parents) ++seen[{0, it.r, it.slot, 0}];
    }
    for (uint64_t i = 0; i < g.chunks; ++i) {  // the chunk check
        const paudit::Item it = paudit::item_of(i, nreq, 1);
        EXPECT(it.r < nreq && it.slot < g.W);
        if (it.slot < pl[it.r].req.last - pl[it.r].req.first) ++seen[{1, it.r, it.slot, 0}];
    }
    for (uint64_t i = 0; i < g.content_units; ++i) {  // the content gather
        const paudit::Item it = paudit::item_of(i, nreq, 64);
        EXPECT(it.r < nreq && it.slot < g.W && it.unit < 64);
        if (1024 * it.slot + 16 * it.unit < pl[it.r].req.olen) ++seen[{2, it.r, it.slot, it.unit}];
    }
    EXPECT(g.extract_units == paudit::extract_items(nreq, g.P, g.W));
    for (uint64_t i = 0; i < g.extract_units; ++i) {  // the proof gather: headers, parents, chunks
        if (i < nreq) {
            if (pl[i].req.last != pl[i].req.first) ++seen[{3, i, 0, 0}];
            continue;
        }
        uint64_t x = i - nreq;
        if (x < 4 * g.P * nreq) {
            const paudit::Item it = paudit::item_of(x, nreq, 4);
            EXPECT(it.r < nreq && it.slot < g.P && it.unit < 4);
            if (it.slot < pl[it.r].parents) ++seen[{4, it.r, it.slot, it.unit}];
            continue;
        }
        x -= 4 * g.P * nreq;
        const paudit::Item it = paudit::item_of(x, nreq, 64);
        EXPECT(it.r < nreq && it.slot < g.W && it.unit < 64);
        if (it.slot < pl[it.r].req.last - pl[it.r].req.first) ++seen[{5, it.r, it.slot, it.unit}];
    }
    uint64_t want = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        const uint64_t w = pl[r].req.last - pl[r].req.first;
        EXPECT(pl[r].parents <= g.P && w <= g.W && pl[r].req.olen <= 1024 * w + (w ? 0 : 1024 * g.W));
        want += pl[r].parents + w + (pl[r].req.olen + 15) / 16 + (w ? 1 : 0) + 4 * pl[r].parents + 64 * w;
        for (uint64_t j = 0; j < pl[r].parents; ++j) {
            EXPECT(seen.count({0, r, j, 0}));
            for (uint64_t u = 0; u < 4; ++u) EXPECT(seen.count({4, r, j, u}));
        }
        for (uint64_t k = 0; k < w; ++k) {
            EXPECT(seen.count({1, r, k, 0}));
            for (uint64_t u = 0; u < 64; ++u) EXPECT(seen.count({5, r, k, u}));
        }
        for (uint64_t o = 0; o < pl[r].req.olen; o += 16) EXPECT(seen.count({2, r, o / 1024, o % 1024 / 16}));
    }
    EXPECT(seen.size() == want);
    for (const auto &kv : seen) EXPECT(kv.second == 1);
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    check_bounds_exhaustive();
    const uintptr_t IN = 0x10000000, OUT = 0x4000000000, PRF = 0x5000000000, HASH = 0x70000000, SCR = 0x7800000000,
                    TAB = 0x7900000000;
    const uint64_t BIG = 1ull << 53;
    uint64_t refused_wide = 0, served = 0;

    // the streams, as the GPU tests pack them: at 56 and 8 mod 256
    std::vector<uint64_t> in_off(NS), in_len(NS), ns(SIZES, SIZES + NS);
    std::vector<uint32_t> padding(NS, 0), chunk_len(NS, 1024);
    uint64_t cur = 0;
    for (uint64_t s = 0; s < NS; ++s) {
        cur = audit::up(cur, 256) + (s % 2 ? 8 : 56);
        in_off[s] = cur;
        in_len[s] = audit::bao_len(SIZES[s]);
        cur += in_len[s];
    }
    chipq_table_info info;
    std::vector<uint8_t> table, rtable;
    EXPECT(qread::plan_table(IN, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), NS, TAB,
                             qread::table_len(NS), &info, &table) == CHIP_OK);
    EXPECT(info.nstreams == NS && info.max_chunks == 66);
    chipp_root_info rinfo;
    EXPECT(paudit::plan_root_table(ns.data(), HASH, NS, TAB, paudit::root_table_len(NS), &rinfo, &rtable) == CHIP_OK);
    EXPECT(rinfo.nroots == NS && rinfo.max_chunks == 66 && rinfo.reserved[0] == 0 && rinfo.reserved[1] == 0);
    const paudit::StreamRec *recs = reinterpret_cast<const paudit::StreamRec *>(table.data());
    const paudit::StreamRec *roots = reinterpret_cast<const paudit::StreamRec *>(rtable.data());
    for (uint64_t s = 0; s < NS; ++s) {
        EXPECT(roots[s].src == 0 && roots[s].n == recs[s].n && roots[s].N == recs[s].N && roots[s].hash == recs[s].hash);
        EXPECT(recs[s].src == IN + in_off[s] && recs[s].n == SIZES[s] && recs[s].hash == HASH + 32 * s);
    }
    // the shift case of the holder's table as the audit kernels read it: stream offsets moved by D, and the base
    // moved by D; the auditor's root table holds no stream address and takes neither
    for (const uint64_t D : plan_shift::SHIFTS) {
        const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D);
        chipq_table_info info2, info3;
        std::vector<uint8_t> by_off, by_base;
        EXPECT(qread::plan_table(IN, in_far.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), NS, TAB,
                                 qread::table_len(NS), &info2, &by_off) == CHIP_OK);
        EXPECT(qread::plan_table(IN + D, in_off.data(), in_len.data(), HASH, padding.data(), chunk_len.data(), NS, TAB,
                                 qread::table_len(NS), &info3, &by_base) == CHIP_OK);
        EXPECT(by_off == by_base && info2.max_chunks == info.max_chunks && info3.nstreams == info.nstreams);
        EXPECT(plan_shift::shifted_words(table, by_off, D) == (long)NS);
        const paudit::StreamRec *far = reinterpret_cast<const paudit::StreamRec *>(by_off.data());
        for (uint64_t s = 0; s < NS; ++s)
            EXPECT(far[s].src == recs[s].src + D && far[s].n == recs[s].n && far[s].N == recs[s].N && far[s].hash == recs[s].hash);
        // a call whose content and proof slots lie past 2^32, base or pitch: the same geometry and scratch
        paudit::Geometry g1, g2, g3;
        paudit::ScratchLayout l1, l2, l3;
        const uint64_t need = paudit::scratch_len(66, 10, 3), pb = audit::up(paudit::proof_bound(66, 3), 16);
        EXPECT(paudit::plan_call(true, TAB, 66, 10, 3, true, OUT, 3072, true, PRF, pb, SCR, need, &g1, &l1) == CHIP_OK);
        EXPECT(paudit::plan_call(true, TAB, 66, 10, 3, true, OUT + D, 3072, true, PRF + D, pb, SCR, need, &g2, &l2) == CHIP_OK);
        EXPECT(paudit::plan_call(true, TAB, 66, 10, 3, true, OUT, D + 256, true, PRF, D + 256, SCR, need, &g3, &l3) == CHIP_OK);
        EXPECT(g1.W == g2.W && g1.W == g3.W && l1.total == l2.total && l1.total == l3.total && l1.total == need);
    }

    for (int round = 0; round < 60; ++round) {
        static const uint64_t COUNTS[] = {1, 2, 3, 8, 70};
        const uint64_t max_count = COUNTS[round % 5];
        const uint64_t nreq = 1 + rng() % 90;
        const uint64_t cstride = 1024 * max_count + 16 * (rng() % 3);
        const uint64_t pstride = audit::up(paudit::proof_bound(info.max_chunks, max_count), 16) + 16 * (rng() % 3);
        const paudit::Shape sh{info.nstreams, info.max_chunks, max_count};
        const paudit::Geometry g(info.max_chunks, nreq, max_count);
        EXPECT(g.ok && g.W == audit::umin(max_count, 66));
        std::vector<uint32_t> rs(nreq);
        std::vector<uint64_t> idx(nreq), cnt(nreq);
        for (uint64_t r = 0; r < nreq; ++r) {
            rs[r] = (uint32_t)(rng() % NS);
            const uint64_t N = audit::chunks(SIZES[rs[r]]);
            switch (rng() % 8) {
            case 0: idx[r] = rng() % N; cnt[r] = 1; break;
            case 1: idx[r] = N + rng() % 3; cnt[r] = 1 + rng() % 3; break;               // an index past the end
            case 2: idx[r] = rng() % (N + 1); cnt[r] = 0; break;                          // a count of 0
            case 3: idx[r] = N - 1 - audit::umin(N - 1, rng() % max_count); cnt[r] = BIG; break;  // clipped at the end
            case 4: idx[r] = rng() % N; cnt[r] = max_count; break;                        // the whole capacity
            case 5: idx[r] = rng() % N; cnt[r] = max_count + 1 + rng() % 2; break;        // perhaps above it
            case 6: idx[r] = BIG; cnt[r] = BIG; break;
            default: idx[r] = rng() % N; cnt[r] = 1 + rng() % (max_count + 1); break;
            }
            if (rng() % 11 == 0) rs[r] = paudit::NO_REQUEST;
        }

        // the device's plan of every request, for the three calls
        std::vector<paudit::Planned> pv(nreq), pe(nreq), pp(nreq);
        std::vector<uint64_t> exact(nreq);
        for (uint64_t r = 0; r < nreq; ++r) {
            pv[r] = paudit::plan_request(recs, sh, paudit::VERIFY, rs[r], idx[r], cnt[r], OUT + r * cstride, 0, 0);
            pe[r] = paudit::plan_request(recs, sh, paudit::EXTRACT, rs[r], idx[r], cnt[r], 0, PRF + r * pstride, 0);
            exact[r] = pe[r].proof_len;
            pp[r] = paudit::plan_request(roots, sh, paudit::PROOFS, rs[r], idx[r], cnt[r], OUT + r * cstride,
                                         PRF + r * pstride, exact[r]);
        }
        check_mapping(pv, g);
        check_mapping(pe, g);
        check_mapping(pp, g);

        // the host plan of the requests the device serves, each at its own slot
        std::vector<uint64_t> keep;
        for (uint64_t r = 0; r < nreq; ++r) {
            if (rs[r] == paudit::NO_REQUEST) {
                EXPECT(pv[r].status == 0 && pe[r].status == 0 && pp[r].status == 0);
            } else {
                const audit::Sel s = audit::select(SIZES[rs[r]], idx[r], cnt[r]);
                const bool wide = s.last - s.first > max_count;
                refused_wide += wide;
                EXPECT(pv[r].status == (wide ? CHIP_ERR_INVALID_ARG : 0) && pe[r].status == pv[r].status &&
                       pp[r].status == pv[r].status);
                if (!wide) keep.push_back(r);
            }
            if (pv[r].status || rs[r] == paudit::NO_REQUEST)
                for (const paudit::Planned *p : {&pv[r], &pe[r], &pp[r]})
                    EXPECT(p->parents == 0 && p->req.first == p->req.last && p->req.olen == 0 && p->proof_len == 0);
        }
        served += keep.size();
        const uint64_t m = keep.size();
        std::vector<uint32_t> hrs(m);
        std::vector<uint64_t> hidx(m), hcnt(m), coff(m), poff(m), plen(m), clen(m), hn(m);
        for (uint64_t j = 0; j < m; ++j) {
            const uint64_t r = keep[j];
            hrs[j] = rs[r]; hidx[j] = idx[r]; hcnt[j] = cnt[r];
            coff[j] = r * cstride; poff[j] = r * pstride; plen[j] = exact[r]; hn[j] = SIZES[rs[r]];
        }
        audit::Plan hv, he, hp;
        EXPECT(audit::plan_verify(false, IN, in_off.data(), in_len.data(), NS, hrs.data(), nullptr, HASH, hidx.data(),
                                  hcnt.data(), m, OUT, coff.data(), clen.data(), true, &hv) == CHIP_OK);
        EXPECT(audit::plan_extract(IN, in_off.data(), in_len.data(), NS, hrs.data(), hidx.data(), hcnt.data(), m, PRF,
                                   poff.data(), plen.data(), &he) == CHIP_OK);  // (a wrong proof_len would be TRUNCATED)
        std::vector<uint64_t> clen2(m);
        EXPECT(audit::plan_verify(true, PRF, poff.data(), plen.data(), m, nullptr, hn.data(), HASH, hidx.data(),
                                  hcnt.data(), m, OUT, coff.data(), clen2.data(), true, &hp) == CHIP_OK);
        for (uint64_t j = 0; j < m; ++j) {
            const uint64_t r = keep[j];
            EXPECT(std::memcmp(&hv.reqs()[j], &pv[r].req, sizeof(audit::Req)) == 0);
            EXPECT(std::memcmp(&he.reqs()[j], &pe[r].req, sizeof(audit::Req)) == 0);
            audit::Req want = hp.reqs()[j];
            EXPECT(want.hash == HASH + 32 * j);      // one hash per REQUEST there, per audited stream here
            want.hash = HASH + 32 * (uint64_t)rs[r];
            EXPECT(std::memcmp(&want, &pp[r].req, sizeof(audit::Req)) == 0);
            const uint64_t par = hv.parents()[j + 1] - hv.parents()[j];
            EXPECT(pv[r].parents == par && pe[r].parents == par && pp[r].parents == par);
            EXPECT(hv.chunks()[j + 1] - hv.chunks()[j] == pv[r].req.last - pv[r].req.first);
            EXPECT(pv[r].req.olen == clen[j] && pp[r].req.olen == clen2[j] && clen[j] == clen2[j]);
            EXPECT(pe[r].proof_len == audit::select(hn[j], hidx[j], hcnt[j]).proof_len && pe[r].proof_len <= pstride);
            EXPECT(he.units()[j + 1] - he.units()[j] == audit::extract_units(par, pe[r].req.last - pe[r].req.first));
            // a proof of the wrong length: status 6, the content length stated, no node read
            const paudit::Planned t = paudit::plan_request(roots, sh, paudit::PROOFS, rs[r], idx[r], cnt[r],
                                                           OUT + r * cstride, PRF + r * pstride, exact[r] + (j % 2 ? 1 : -1));
            EXPECT(t.status == CHIP_ERR_BAO_TRUNCATED && t.req.olen == clen[j] && t.req.dst == OUT + r * cstride);
            EXPECT(t.parents == 0 && t.req.first == t.req.last);
        }

        // requests the device refuses
        const struct { uint32_t s; uint64_t index, count; } bad[] = {
            {(uint32_t)NS, 0, 1}, {0xFFFFFFFEu, 0, 1}, {NS - 1, BIG + 1, 1}, {NS - 1, 0, BIG + 1}, {NS - 1, 0, max_count + 1}};
        for (const auto &b : bad)
            if (b.count <= 66 || b.count > BIG)  // (a selection above max_count, not above the stream)
                for (paudit::Kind k : {paudit::VERIFY, paudit::EXTRACT, paudit::PROOFS}) {
                    const paudit::Planned p = paudit::plan_request(recs, sh, k, b.s, b.index, b.count, OUT, PRF, 8);
                    EXPECT(p.status == CHIP_ERR_INVALID_ARG && p.parents == 0 && p.req.first == p.req.last &&
                           p.req.olen == 0 && p.proof_len == 0);
                }
        paudit::Shape lie = sh;
        lie.max_chunks = info.max_chunks - 1;  // an info that is not the table's
        for (uint32_t s = 0; s < NS; ++s) {
            const paudit::Planned p = paudit::plan_request(recs, lie, paudit::VERIFY, s, 0, 1, OUT, 0, 0);
            EXPECT((p.status == CHIP_ERR_INVALID_ARG) == (recs[s].N == info.max_chunks));
        }
    }
    std::printf("%llu requests served, %llu above the capacity\n", (unsigned long long)served,
                (unsigned long long)refused_wide);
    EXPECT(served > 500 && refused_wide > 20);

    // the host checks of the root table, in the header's order
    {
        chipp_root_info ri{9, 9, {9, 9}};
        std::vector<uint8_t> t;
        const uint64_t need = paudit::root_table_len(3);
        const uint64_t n3[] = {0, 5000, 1ull << 62}, over[] = {0, (1ull << 62) + 1, 5};
        auto zero = [&] { return ri.nroots == 0 && ri.max_chunks == 0 && ri.reserved[0] == 0 && ri.reserved[1] == 0; };
        EXPECT(need % 16 == 0 && need >= 3 * sizeof(paudit::StreamRec) && paudit::root_table_len(1ull << 32) == 0);
        EXPECT(paudit::plan_root_table(n3, HASH, 3, TAB, need, nullptr, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(nullptr, HASH, 3, TAB, need, &ri, &t) == CHIP_ERR_INVALID_ARG && zero());
        EXPECT(paudit::plan_root_table(n3, HASH, 3, 0, need, &ri, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(n3, HASH, 3, TAB + 8, need, &ri, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(n3, HASH, 1ull << 32, TAB, ~0ull, &ri, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(over, HASH, 3, TAB, need, &ri, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(n3, HASH, 3, TAB, need - 1, &ri, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(n3, 0, 3, TAB, need, &ri, &t) == CHIP_ERR_HASH_DECODE && zero());
        EXPECT(paudit::plan_root_table(n3, 0, 3, TAB, need - 1, &ri, &t) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::plan_root_table(over, 0, 3, TAB, need, &ri, &t) == CHIP_ERR_INVALID_ARG && t.empty());
        EXPECT(paudit::plan_root_table(n3, HASH, 3, TAB, need, &ri, &t) == CHIP_OK && ri.nroots == 3 &&
               ri.max_chunks == (1ull << 52) && t.size() == need);
        EXPECT(paudit::plan_root_table(nullptr, HASH, 0, TAB, 0, &ri, &t) == CHIP_OK && zero() && t.empty());
    }

    // the host checks of a call, in the header's order
    {
        paudit::Geometry g;
        paudit::ScratchLayout lay;
        const uint64_t MC = 66, need = paudit::scratch_len(MC, 10, 3), pb = audit::up(paudit::proof_bound(MC, 3), 16);
        auto call = [&](bool have, uintptr_t tab, uint64_t nreq, uint64_t max_count, uintptr_t out, uint64_t cs,
                        uintptr_t prf, uint64_t ps, uintptr_t scr, uint64_t sl) {
            return paudit::plan_call(have, tab, MC, nreq, max_count, true, out, cs, true, prf, ps, scr, sl, &g, &lay);
        };
        EXPECT(need && need % 16 == 0 && need >= 10 * (sizeof(audit::Req) + 8));
        EXPECT(call(false, 0, 0, 0, 0, 7, 0, 7, 0, 0) == CHIP_OK);
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF, pb, SCR, need) == CHIP_OK && g.W == 3 && lay.total == need);
        EXPECT(call(false, TAB, 10, 3, OUT, 3072, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 1ull << 31, 3, OUT, 3072, PRF, pb, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 0, OUT, 3072, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, (1ull << 53) + 1, OUT, 1ull << 60, PRF, 1ull << 60, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 3, OUT, 3080, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);   // no multiple of 16
        EXPECT(call(true, TAB, 10, 3, OUT, 3056, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);   // below 1024 max_count
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF, pb - 16, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF, pb + 8, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 3, OUT, 1ull << 62, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);  // a slot address wraps
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF, 1ull << 62, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 3, OUT + 8, 3072, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF + 8, pb, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB + 8, 10, 3, OUT, 3072, PRF, pb, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF, pb, SCR + 8, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(true, TAB, 1 << 30, 66, OUT, 66 * 1024, PRF, audit::up(paudit::proof_bound(MC, 66), 16), SCR, ~0ull) ==
               CHIP_ERR_INVALID_ARG);  // 2^36 work items
        EXPECT(call(true, TAB, 10, 3, OUT, 3072, PRF, pb, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
        EXPECT(paudit::scratch_len(MC, 1 << 30, 66) == 0 && paudit::scratch_len(MC, 1ull << 31, 1) == 0);
        EXPECT(paudit::scratch_len(MC, 10, 0) == 0 && paudit::scratch_len(MC, 10, (1ull << 53) + 1) == 0);
        EXPECT(paudit::scratch_len(MC, 10, 1ull << 53) == need);  // no request selects more chunks than its stream has
        // a call without proofs does not look at the proof arguments, one without content not at the content's
        EXPECT(paudit::plan_call(true, TAB, MC, 10, 3, true, OUT, 3072, false, 0, 7, SCR, need, &g, &lay) == CHIP_OK);
        EXPECT(paudit::plan_call(true, TAB, MC, 10, 3, false, 0, 7, true, PRF, pb, SCR, need, &g, &lay) == CHIP_OK);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
