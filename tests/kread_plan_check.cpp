// kread_plan_check.cpp — the device-planned plaintext reads of level-13 objects
// (carbonado_amd/csrc/kread_device.hpp, the text kread_kernels.hip runs,
// compiled here as host code, and kread_plan.hpp, the host's O(1) share) driven
// stand-alone, for a build with -fsanitize=address,undefined
// (tests/test_kread_cpu.py).  No device: the addresses are made-up integers.
//
//  * the rewrite: over seeded requests kread::decide's envelope request is
//    cread::shifted's, and its decision (refused, killed, read) is the one the
//    host call makes for that request alone (vread::plan_vread over the shifted
//    request, the capacity, cread::plan_ctr over the plaintext range, then
//    key_status); the rewritten request through qread::plan_request gives the
//    host plan's content length, 1 with no work where it is refused and no work
//    where it is killed.  Among the requests: the limits 2^53 - 97, 2^53 - 96
//    and 2^36 - 32, a stream with n < 97 and key_status 0, stream indices at
//    and past nstreams, an info that is not the table's;
//  * the bounded work mapping: for seeded (pos, n, max_len), n <= max_len,
//    walking every wave and lane of the cap-sized grid touches every unit of
//    the item exactly once and no byte past n (the buffer ends at byte n), and
//    lane_eval / lane_apply give the bytes of the host-planned item split
//    (cread::plan_ctr, cread::item_of) that tests/cread_device_check.cpp walks;
//    a killed request's waves zero exactly [0, n);
//  * the key table's layout and upload, the host checks in their order, and the
//    scratch layout's regions.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/kread_plan.hpp"
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
                       KEYS = 0x7A00000000;

// ---- the rewrite ---------------------------------------------------------------------
struct World {
    uint64_t nstreams;
    std::vector<uint64_t> in_off, in_len;
    std::vector<uint32_t> chunk_len, padding, key_status;
    std::vector<uint8_t> keys, ivs, table;
    chipq_table_info info;
    const qread::StreamRec *recs() const { return reinterpret_cast<const qread::StreamRec *>(table.data()); }
};

// what the host call decides for one request alone: 1 refused, 2 killed, 3 read; *clen its content length
static uint32_t host_decision(const World &w, uint32_t stream, uint64_t start, uint64_t len, uint64_t max_len,
                              uint64_t *clen, uint32_t *status) {
    const std::vector<uint64_t> sh = cread::shifted(&start, 1);
    const uint64_t coff = 0;
    *clen = 0;
    *status = 0;
    vread::Plan vp;
    const int vst = vread::plan_vread(IN, w.in_off.data(), w.in_len.data(), HASH, w.padding.data(), w.chunk_len.data(),
                                      w.nstreams, &stream, sh.data(), &len, 1, OUT, &coff, clen, true, 0, SCR, ~0ull, &vp);
    if (vst != CHIP_OK) {
        EXPECT(vst == CHIP_ERR_INVALID_ARG);
        *clen = 0;
        return kread::REFUSED;
    }
    if (*clen > max_len) return kread::REFUSED;  // the capacity: the device's own check, as in qread
    const uint32_t kill = w.key_status[stream];
    cread::Plan cp;
    const int cst = cread::plan_ctr(w.keys.data(), w.ivs.data(), w.nstreams, &stream, &start, clen, 1, OUT, &coff, SCR,
                                    ~0ull, &kill, &cp);
    if (cst != CHIP_OK) return kread::REFUSED;
    *status = vp.rd.reqs()[0].status;
    return kill ? kread::KILLED : kread::READ;
}

static void check_rewrite(std::mt19937_64 &rng) {
    const uint32_t shard[] = {1024, 2048, 4096, 65536};
    uint64_t seen[4] = {0, 0, 0, 0};
    for (int round = 0; round < 60; ++round) {
        World w;
        w.nstreams = 7 + rng() % 4;
        const uint64_t ns = w.nstreams;
        w.in_off.resize(ns); w.in_len.resize(ns); w.chunk_len.resize(ns); w.padding.resize(ns);
        w.key_status.assign(ns, 0);
        w.keys.assign(32 * ns, 0x5A); w.ivs.assign(16 * ns, 0xA5);
        uint64_t cur = 56;
        for (uint64_t s = 0; s < ns; ++s) {
            const uint32_t C = s < 4 ? shard[s] : shard[rng() % 4];
            w.chunk_len[s] = C;
            w.padding[s] = s % 2 ? 0 : (uint32_t)(rng() % (4 * C - 200));
            w.in_off[s] = cur;
            w.in_len[s] = audit::bao_len(8ull * C);
            cur += audit::up(w.in_len[s], 8) + 8 * (rng() % 4);
        }
        w.chunk_len[4] = w.chunk_len[4] == 1024 ? 2048 : 1024;   // a chunk_len that does not fit its stream's length
        w.padding[5] = 4 * w.chunk_len[5] - (uint32_t)(rng() % 97);  // an object shorter than an envelope, key_status 0
        w.key_status[6] = 17;                                     // a killed stream
        if (round % 3 == 0) w.key_status[4] = 7;                  // killed and unservable
        EXPECT(qread::plan_table(IN, w.in_off.data(), w.in_len.data(), HASH, w.padding.data(), w.chunk_len.data(), ns, TAB,
                                 qread::table_len(ns), &w.info, &w.table) == CHIP_OK);
        const uint64_t max_len = round % 2 ? 5000 : 4096;
        const kread::Geometry g(w.info, 64, max_len);
        EXPECT(g.ok && g.cap == cread::spans_of(max_len));
        const qread::Shape sh{w.info.nstreams, w.info.max_chunks, w.info.min_shard, max_len, g.q.S};

        struct R { uint32_t s; uint64_t start, len; };
        std::vector<R> reqs;
        const uint64_t top = 1ull << 53, gend = cread::MAX_END;
        for (uint32_t s = 0; s <= ns + 1; ++s) {  // the limits on every stream, and on indices at and past nstreams
            const uint32_t idx = s == ns + 1 ? ~0u : s;
            const std::vector<uint64_t> starts = {0, 1, top - 98, top - 97, top - 96, top, top + 1, gend - 1, gend,
                                                  gend + 1, gend - 4096, ~0ull, ~0ull - 96, ~0ull - 97};
            const std::vector<uint64_t> lens = {0, 1, 4096, max_len, max_len + 1, top, top + 1, ~0ull};
            for (uint64_t st : starts)
                for (uint64_t ln : lens)
                    reqs.push_back(R{idx, st, ln});
        }
        for (int i = 0; i < 400; ++i) {
            const uint32_t s = (uint32_t)(rng() % ns);
            const uint64_t n_obj = 4ull * w.chunk_len[s] - w.padding[s], P = n_obj > 97 ? n_obj - 97 : 0;
            R q{s, 0, 0};
            switch (rng() % 6) {
            case 0: q.start = rng() % (P + 10); q.len = rng() % 64; break;
            case 1: q.start = w.chunk_len[s] * (1 + rng() % 3) - 97 - rng() % 100; q.len = 200; break;  // across a shard boundary
            case 2: q.start = rng() % (P + 1); q.len = max_len + rng() % 3; break;
            case 3: q.start = P - audit::umin(P, rng() % 3000); q.len = 1ull << 40; break;            // clipped at P
            case 4: q.start = P + rng() % 5; q.len = 7; break;                                         // at or past P
            default: q.start = rng() % (P + 1); q.len = rng() % (max_len + 1); break;
            }
            reqs.push_back(q);
        }

        std::vector<read::Req> preq(1);
        std::vector<read::Seg> segs(g.q.S);
        std::vector<audit::Req> slices(g.q.S);
        std::vector<uint64_t> pre[4], qlen(1);
        for (auto &a : pre) a.assign(g.q.S + 1, ~0ull);
        const qread::Tables t{preq.data(), segs.data(), slices.data(), pre[0].data(), pre[1].data(), pre[2].data(),
                              pre[3].data(), qlen.data()};
        for (const R &q : reqs) {
            const kread::Decision d = kread::decide(w.recs(), w.key_status.data(), sh, q.s, q.start, q.len);
            uint64_t clen = 0;
            uint32_t status = 0;
            const uint32_t want = host_decision(w, q.s, q.start, q.len, max_len, &clen, &status);
            EXPECT(d.order == want);
            ++seen[want];
            if (want != kread::REFUSED) {
                EXPECT(d.q_stream == q.s && d.q_start == cread::shifted(&q.start, 1)[0]);
                EXPECT(d.q_start == q.start + 97);
            } else {
                EXPECT(d.q_stream == kread::NO_STREAM && d.q_stream >= sh.nstreams);
            }
            if (want == kread::KILLED) EXPECT(d.kill == w.key_status[q.s] && d.clen == clen && d.q_len == 0);
            if (want == kread::READ) EXPECT(d.kill == 0 && d.q_len == q.len);
            // what KQ's planner makes of the rewritten request
            qread::plan_request(w.recs(), sh, 0, d.q_stream, d.q_start, d.q_len, OUT, t);
            bool work = false;
            for (auto &a : pre)
                for (uint32_t k = 0; k < g.q.S; ++k) work |= a[k] != 0;
            if (want == kread::REFUSED) EXPECT(preq[0].status == CHIP_ERR_INVALID_ARG && qlen[0] == 0 && !work);
            if (want == kread::KILLED) EXPECT(qlen[0] == 0 && !work && preq[0].nseg == 0);
            if (want == kread::READ) EXPECT(preq[0].status == status && qlen[0] == clen && work == (clen != 0));
        }
        // a stream shorter than an envelope, key_status 0: an empty plaintext, status 0
        {
            const kread::Decision d = kread::decide(w.recs(), w.key_status.data(), sh, 5, 0, 100);
            qread::plan_request(w.recs(), sh, 0, d.q_stream, d.q_start, d.q_len, OUT, t);
            EXPECT(d.order == kread::READ && preq[0].status == 0 && qlen[0] == 0);
        }
        // an info that is not the table's
        qread::Shape lie = sh;
        lie.max_chunks = w.info.max_chunks - 1;
        for (uint32_t s = 0; s < ns; ++s) {
            const kread::Decision d = kread::decide(w.recs(), w.key_status.data(), lie, s, 0, 10);
            EXPECT((d.order == kread::REFUSED) == (w.recs()[s].N == w.info.max_chunks));
        }
        lie = sh;
        lie.min_shard = 2048;
        EXPECT(kread::decide(w.recs(), w.key_status.data(), lie, 0, 0, 10).order == kread::REFUSED);
    }
    std::printf("decisions: %llu refused, %llu killed, %llu read\n", (unsigned long long)seen[1],
                (unsigned long long)seen[2], (unsigned long long)seen[3]);
    EXPECT(seen[1] > 100 && seen[2] > 100 && seen[3] > 100);
}

// ---- the bounded work mapping -----------------------------------------------------------
static cread::CtrKey make_key(std::mt19937_64 &rng) {
    uint8_t raw[48];
    for (auto &b : raw) b = (uint8_t)rng();
    cread::CtrKey k{};
    uint32_t w[60];
    gcm::aes256_expand(raw, w, k.rk);
    cread::setup_lite(k.rk, raw + 32, k.j0);
    return k;
}

// one wave: lane_eval for the 64 lanes, the neighbour exchange, lane_apply
static void wave(const cread::CtrKey &k, const cread::Item &it, uint32_t span, uint8_t *buf) {
    using namespace cread;
    uint32_t ka[LANES + 1][4], kb[LANES][4];
    for (uint32_t l = 0; l < LANES; ++l) {
        for (int j = 0; j < 4; ++j) ka[l][j] = kb[l][j] = 0;
        if (lane_needed(it, span, l)) lane_eval(&k, it, span, l, ka[l], kb[l]);
    }
    for (int j = 0; j < 4; ++j) ka[LANES][j] = 0xDEADBEEFu;  // what lane 63's shuffle reads is not defined
    for (uint32_t l = 0; l < LANES; ++l) lane_apply(it, span, l, ka[l], kb[l], ka[l + 1], buf);
}

static void check_mapping(std::mt19937_64 &rng) {
    using namespace cread;
    const CtrKey key = make_key(rng);
    const uint64_t span_bytes = 16ull * SPAN_UNITS;
    std::vector<uint64_t> lens = {0, 1, 15, 16, 17, 2031, 2032, 2033, 4064, 4096, 5000, 2 * span_bytes + 1};
    for (int i = 0; i < 24; ++i) lens.push_back(rng() % 9000);
    for (uint64_t n : lens)
        for (uint64_t max_len : {n ? n : 1, (uint64_t)4096, (uint64_t)5000, n + 1 + rng() % 6000, 4 * span_bytes}) {
            if (n > max_len) continue;
            const uint32_t cap = kread::span_cap(max_len);
            const uint64_t pos = rng() % 4 ? rng() % (1ull << 20) : MAX_END - n - rng() % 16;  // (up to the cipher's limit)
            const uint32_t r = (uint32_t)(rng() % 5);
            const uint64_t stride = read::up(max_len, 16);
            // the buffer ends at byte n of the request's slot: a byte past n is a sanitizer report
            std::vector<uint8_t> plain(n), got(n), ref(n);
            for (auto &b : plain) b = (uint8_t)rng();
            got = plain;
            ref = plain;
            std::vector<uint32_t> touched(units_of(n), 0);
            uint64_t waves = 0;
            for (uint32_t w = r * cap; w < (r + 1) * cap; ++w) {  // request r's share of the nreq * cap grid
                EXPECT(w / cap == r);
                const uint32_t span = w % cap;
                const Item it = kread::item_of_request(r, stride, pos, n, 0, 0);
                EXPECT(it.buf_off == r * stride);
                if (span >= spans_of(it.n)) continue;  // leaves at once
                ++waves;
                const uint32_t nu = span_units(it, span);
                for (uint32_t l = 0; l < LANES; ++l)
                    for (uint32_t j = 0; j < 2; ++j) {
                        const uint32_t x = 2 * l + j;
                        if (x < nu && x < SPAN_UNITS) ++touched[span * SPAN_UNITS + x];
                    }
                wave(key, it, span, got.data());
            }
            EXPECT(waves == spans_of(n) && waves <= cap);
            for (uint32_t c : touched) EXPECT(c == 1);
            // the host-planned split of the same item
            const uint32_t ik = 0;
            const uint64_t off = 0;
            uint8_t k32[32] = {}, iv16[16] = {};
            alignas(16) static uint8_t anchor[16];
            Plan p;
            EXPECT(plan_ctr(k32, iv16, 1, &ik, &pos, &n, 1, reinterpret_cast<uintptr_t>(anchor), &off,
                            reinterpret_cast<uintptr_t>(anchor), ~0ull, nullptr, &p) == CHIP_OK);
            const Item *items = reinterpret_cast<const Item *>(p.table.data() + p.lay.items);
            EXPECT(p.work == spans_of(n));
            for (uint64_t w = 0; w < p.work; ++w) {
                const Item it = items[item_of(items, 1, (uint32_t)w)];
                wave(key, it, (uint32_t)w - it.work0, ref.data());
            }
            EXPECT(got == ref);
            if (n >= 64) EXPECT(got != plain);
            for (uint32_t w = 0; w < cap; ++w) {  // applied twice it is the identity
                const Item it = kread::item_of_request(0, stride, pos, n, 0, 0);
                if (w < spans_of(n)) wave(key, it, w, got.data());
            }
            EXPECT(got == plain);
            // a killed request: zeros over [0, n) from the same grid; an empty one still has span 0
            const Item kit = kread::item_of_request(r, stride, pos, n, 0, 17);
            uint64_t kwaves = 0;
            for (uint32_t span = 0; span < cap; ++span) {
                if (span >= work_of(kit.n, kit.kill)) continue;
                ++kwaves;
                for (uint32_t l = 0; l < LANES; ++l) lane_zero(kit, span, l, got.data());
            }
            EXPECT(kwaves == work_of(n, 17) && kwaves >= 1 && kwaves <= cap);
            for (uint8_t b : got) EXPECT(b == 0);
        }
}

// ---- the host's share ------------------------------------------------------------------------
static void check_host() {
    // the key table
    EXPECT(kread::table_len(0) == 0 && kread::table_len(1ull << 32) == 0);
    for (uint64_t ns : {1ull, 2ull, 3ull, 4ull, 5ull, 1024ull, (1ull << 32) - 1}) {
        const kread::TableLayout l(ns);
        EXPECT(l.km == 0 && l.status == 512 * ns && l.raw >= l.status + 4 * ns && l.total == l.raw + 48 * ns);
        EXPECT(l.status % 16 == 0 && l.raw % 16 == 0 && l.total % 16 == 0 && kread::table_len(ns) == l.total);
        EXPECT(l.upload_len() == l.total - l.status);
    }
    EXPECT(kread::check_table(false, false, 0, 0, 0) == CHIP_OK);
    const uint64_t need3 = kread::table_len(3);
    EXPECT(kread::check_table(true, true, KEYS, 3, need3) == CHIP_OK);
    EXPECT(kread::check_table(false, true, KEYS, 3, need3) == CHIP_ERR_INVALID_ARG);
    EXPECT(kread::check_table(true, false, KEYS, 3, need3) == CHIP_ERR_INVALID_ARG);
    EXPECT(kread::check_table(true, true, 0, 3, need3) == CHIP_ERR_INVALID_ARG);
    EXPECT(kread::check_table(true, true, KEYS + 8, 3, need3) == CHIP_ERR_INVALID_ARG);
    EXPECT(kread::check_table(true, true, KEYS, 1ull << 32, ~0ull) == CHIP_ERR_INVALID_ARG);
    EXPECT(kread::check_table(true, true, KEYS, 3, need3 - 1) == CHIP_ERR_INVALID_ARG);
    {
        std::vector<uint8_t> keys(96), ivs(48);
        for (size_t i = 0; i < keys.size(); ++i) keys[i] = (uint8_t)(i + 1);
        for (size_t i = 0; i < ivs.size(); ++i) ivs[i] = (uint8_t)(200 - i);
        const uint32_t ks[3] = {0, 17, 0};
        const kread::TableLayout l(3);
        const std::vector<uint8_t> up = kread::table_upload(keys.data(), ivs.data(), ks, 3);
        EXPECT(up.size() == l.upload_len());
        EXPECT(std::memcmp(up.data(), ks, 12) == 0);
        const uint8_t *raw = up.data() + (l.raw - l.status);
        EXPECT(std::memcmp(raw, keys.data(), 32) == 0 && std::memcmp(raw + 32, ivs.data(), 16) == 0);
        for (int i = 0; i < 48; ++i) EXPECT(raw[48 + i] == 0);  // the killed stream's key never leaves the host
        EXPECT(std::memcmp(raw + 96, keys.data() + 64, 32) == 0 && std::memcmp(raw + 128, ivs.data() + 32, 16) == 0);
        const std::vector<uint8_t> all = kread::table_upload(keys.data(), ivs.data(), nullptr, 3);
        EXPECT(std::memcmp(all.data() + (l.raw - l.status) + 48, keys.data() + 32, 32) == 0);
        for (int i = 0; i < 12; ++i) EXPECT(all[i] == 0);
    }

    // the scratch: qread's vouched scratch, then the three request arrays, nothing overlapping
    chipq_table_info info{3, 512, 1024, 0};
    for (uint64_t nreq : {1ull, 10ull, 63ull, 64ull, 65ull, 257ull, 16384ull})
        for (uint64_t max_len : {1ull, 4096ull, 5000ull, 70000ull}) {
            const kread::Geometry g(info, nreq, max_len);
            EXPECT(g.ok && g.cap == cread::spans_of(max_len) && g.work == nreq * g.cap);
            const kread::ScratchLayout lay(g, nreq);
            EXPECT(lay.q.total == qread::scratch_len(&info, nreq, max_len, true));
            EXPECT(lay.q_stream >= lay.q.total && lay.q_start >= lay.q_stream + 4 * nreq);
            EXPECT(lay.q_len >= lay.q_start + 8 * nreq && lay.total >= lay.q_len + 8 * nreq);
            EXPECT(lay.q_stream % 256 == 0 && lay.q_start % 256 == 0 && lay.q_len % 256 == 0 && lay.total % 16 == 0);
            EXPECT(kread::scratch_len(&info, nreq, max_len) == lay.total);
            EXPECT(kread::scratch_len(&info, nreq + 64, max_len) > lay.total);
        }
    EXPECT(kread::scratch_len(nullptr, 1, 1) == 0 && kread::scratch_len(&info, 1ull << 31, 4096) == 0);
    EXPECT(kread::scratch_len(&info, 16, 0) == 0 && kread::scratch_len(&info, 16, (1ull << 53) + 1) == 0);
    EXPECT(kread::scratch_len(&info, 1 << 30, 1ull << 20) == 0);
    // 2^31 keystream waves where qread's own bounds still hold
    {
        chipq_table_info big{3, 8, 1ull << 30, 0};
        const uint64_t nreq = 1ull << 20, max_len = 4ull << 20;  // 2^20 requests of 2065 spans each
        EXPECT(qread::scratch_len(&big, nreq, max_len, true) != 0 && kread::scratch_len(&big, nreq, max_len) == 0);
        EXPECT(kread::scratch_len(&big, nreq / 2, max_len) != 0);
    }

    // the host checks of a read call, in the header's order
    kread::Geometry g;
    kread::ScratchLayout lay;
    const uint64_t need = kread::scratch_len(&info, 10, 4096), tlen = kread::table_len(3);
    auto call = [&](uintptr_t tab, const chipq_table_info *i, uintptr_t kt, uint64_t kl, bool reqs, uint64_t nreq,
                    uint64_t max_len, uintptr_t out, uint64_t stride, bool res, uint32_t flags, uintptr_t scr,
                    uint64_t sl) {
        return kread::plan_call(tab, i, kt, kl, reqs, nreq, max_len, out, stride, res, flags, scr, sl, &g, &lay);
    };
    EXPECT(need && need % 16 == 0 && need > qread::scratch_len(&info, 10, 4096, true));
    EXPECT(call(0, nullptr, 0, 0, false, 0, 0, 0, 0, false, 9, 0, 0) == CHIP_OK);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 1, SCR, need) == CHIP_OK);
    EXPECT(lay.total == need && g.cap == 3);
    // the shift case: the key table holds no address and the stream table is qread's (tests/qread_plan_check.cpp);
    // what a call takes is the content base and stride, past 2^32 here: the same verdict, geometry and scratch
    for (const uint64_t D : plan_shift::SHIFTS) {
        EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT + D, 4096, true, 1, SCR, need) == CHIP_OK);
        EXPECT(lay.total == need && g.cap == 3);
        EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, D + 256, true, 1, SCR, need) == CHIP_OK);
        EXPECT(lay.total == need && g.cap == 3);
        EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT + D, D + 264, true, 1, SCR, need) == CHIP_ERR_INVALID_ARG);
    }
    EXPECT(call(0, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, nullptr, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, 0, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, false, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, false, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 1ull << 31, 4096, OUT, 4096, true, 0, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 0, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, 4088, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT + 8, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB + 8, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS + 8, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen - 1, true, 10, 4096, OUT, 4096, true, 0, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 2, SCR, need) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 1 << 30, 1ull << 20, OUT, 1ull << 20, true, 0, SCR, ~0ull) ==
           CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR, need - 1) == CHIP_ERR_INVALID_ARG);
    EXPECT(call(TAB, &info, KEYS, tlen, true, 10, 4096, OUT, 4096, true, 0, SCR,
                qread::scratch_len(&info, 10, 4096, true)) == CHIP_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    check_rewrite(rng);
    check_mapping(rng);
    check_host();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
