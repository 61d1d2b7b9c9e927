// repair_plan_check.cpp — the host logic of the ragged scrub
// (carbonado_amd/csrc/repair_plan.hpp: argument checks, scratch layout,
// verdict requests, per-object statuses, passes, records) driven stand-alone,
// for a build with -fsanitize=address,undefined (tests/test_repair_cpu.py).
// No device: the addresses are made-up integers, nothing is dereferenced.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/repair_plan.hpp"
#include "plan_shift.hpp"

using namespace chip;
using namespace chip::repair;

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

// regions sorted by start are disjoint and end at or before `limit`
static void expect_disjoint(std::vector<Region> r, uint64_t limit) {
    std::sort(r.begin(), r.end(), [](const Region &a, const Region &b) { return a.lo < b.lo; });
    for (size_t i = 0; i < r.size(); ++i) {
        EXPECT(r[i].lo <= r[i].hi && r[i].hi <= limit);
        if (i) EXPECT(r[i - 1].hi <= r[i].lo);
    }
}

// all 70 four-subsets of 8: the record's coefficients times the selected rows
// of the encoding matrix are the identity
static void check_inverses() {
    const Gf256 &g = Gf256::get();
    const std::vector<uint8_t> enc = zfec_enc_matrix(4, 8);
    int subsets = 0;
    for (uint32_t m = 0; m < 256; ++m) {
        if (__builtin_popcount(m) != 4) continue;
        ++subsets;
        uint8_t sel[4], coef[16];
        uint32_t k = 0;
        for (uint32_t i = 0; i < 8; ++i)
            if (m >> i & 1) sel[k++] = (uint8_t)i;
        EXPECT(inverse_for(sel, coef));
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                uint8_t acc = 0;
                for (int s = 0; s < 4; ++s) acc ^= g.mul(coef[4 * r + s], enc[4 * sel[s] + c]);
                EXPECT(acc == (r == c ? 1 : 0));
            }
        for (int s = 0; s < 4; ++s)  // a selected primary: a unit row, a plain copy
            if (sel[s] < 4)
                for (int t = 0; t < 4; ++t) EXPECT(coef[4 * sel[s] + t] == (t == s ? 1 : 0));
    }
    EXPECT(subsets == 70);
    const uint8_t bad[4] = {0, 1, 2, 9};
    uint8_t coef[16];
    EXPECT(!inverse_for(bad, coef));
}

static void check_statuses() {
    const uint64_t C = 3072, n = 8 * C, len = audit::bao_len(n);
    const uint32_t pad = 40;
    EXPECT(pre_status(len, n, C, pad, 0xFF) == CHIP_ERR_UNNECESSARY_SCRUB);
    EXPECT(pre_status(len, n, C, pad, 0x07) == CHIP_ERR_ZFEC);
    EXPECT(pre_status(len, n, C, pad, 0x0F) == -1 && pre_status(len, n, C, pad, 0xFE) == -1);
    EXPECT(pre_status(len, n, 0, pad, 0xFE) == CHIP_ERR_ZFEC);
    EXPECT(pre_status(len, n, C + 1, pad, 0xFE) == CHIP_ERR_ZFEC);
    EXPECT(pre_status(len, n, 2048, pad, 0xFE) == CHIP_ERR_ZFEC);
    EXPECT(pre_status(len, n, C, 4 * C + 1, 0xFE) == CHIP_ERR_ZFEC);
    EXPECT(pre_status(len, n, C, 4096 + pad, 0xFE) == CHIP_ERR_SCRUBBED_PADDING_MISMATCH);
    EXPECT(pre_status(len, n, C, 4 * C, 0xFE) == CHIP_ERR_SCRUBBED_PADDING_MISMATCH);
    EXPECT(pre_status(len, n, C, 0, 0xFE) == -1 && pre_status(len, n, C, 4095, 0xFE) == -1);
}

// the verdicts behind the mask in their order: too few shares, padding out of
// range, padding mismatch, length mismatch, and only then a repair; an earlier
// cause hides every later one
static void check_verdicts() {
    using chip::rules::REPAIR;
    using chip::rules::scrub_verdict;
    int cases = 0;
    for (uint64_t spc : {1, 2, 3, 7, 64, 1000})
        for (uint32_t pad : {0u, 1u, 40u, 4095u}) {
            const uint64_t C = 1024 * spc, len = audit::bao_len(8 * C);
            const uint64_t other[3] = {len + 8, len - 8, audit::bao_len(8 * (C + 1024))};  // not this stream's length
            const uint32_t off_range[2] = {(uint32_t)(4 * C + 1), ~0u};                     // padding > 4 C
            const uint32_t mismatch[3] = {pad + 4096, (uint32_t)(4 * C), pad + 8192};        // <= 4 C, not what zfec pads
            for (uint32_t good = 0; good <= 8; ++good) {
                const bool few = good < 4;
                EXPECT(scrub_verdict(len, C, pad, good) == (few ? CHIP_ERR_ZFEC : REPAIR));
                for (uint32_t bad : off_range) {
                    EXPECT(scrub_verdict(len, C, bad, good) == CHIP_ERR_ZFEC);
                    for (uint64_t l : other) EXPECT(scrub_verdict(l, C, bad, good) == CHIP_ERR_ZFEC);
                }
                for (uint32_t bad : mismatch) {
                    if (bad > 4 * C) continue;  // (one chunk per shard: the larger ones are out of range instead)
                    const int want = few ? CHIP_ERR_ZFEC : CHIP_ERR_SCRUBBED_PADDING_MISMATCH;
                    EXPECT(scrub_verdict(len, C, bad, good) == want);
                    for (uint64_t l : other) EXPECT(scrub_verdict(l, C, bad, good) == want);
                }
                for (uint64_t l : other)
                    EXPECT(scrub_verdict(l, C, pad, good) == (few ? CHIP_ERR_ZFEC : CHIP_ERR_SCRUBBED_LENGTH_MISMATCH));
                ++cases;
            }
            // what pre_status decides in front of them, and that it hands the rest on unchanged
            EXPECT(pre_status(len, 8 * C, (uint32_t)C, pad, 0xFF) == CHIP_ERR_UNNECESSARY_SCRUB);
            EXPECT(pre_status(len + 8, 8 * C, (uint32_t)C, pad, 0x3C) == CHIP_ERR_SCRUBBED_LENGTH_MISMATCH);
            EXPECT(pre_status(len + 8, 8 * C, (uint32_t)C + 1024, pad, 0x3C) == CHIP_ERR_ZFEC);
        }
    EXPECT(cases == 6 * 4 * 9);
}

static void check_overlaps() {
    const uintptr_t IN = 0x10000000, OUT = 0x80000000;
    const uint64_t len[2] = {audit::bao_len(8192), audit::bao_len(16384)};
    const uint64_t in_off[2] = {56, 65536 + 8};
    uint64_t out_off[2] = {0, 32768};
    EXPECT(!bad_overlap(IN, in_off, OUT, out_off, len, 2));
    EXPECT(!bad_overlap(IN, in_off, IN, in_off, len, 2));  // in place: every range its own
    out_off[1] = len[0] - 8;
    EXPECT(bad_overlap(IN, in_off, OUT, out_off, len, 2));  // two outputs
    uint64_t shifted[2] = {in_off[0] + 8, in_off[1]};
    EXPECT(bad_overlap(IN, in_off, IN, shifted, len, 2));  // an output over part of its own input
    uint64_t swapped[2] = {in_off[1], 1 << 20};
    EXPECT(bad_overlap(IN, in_off, IN, swapped, len, 2));  // an output over another object's input
    uint64_t mixed[2] = {in_off[0], 1 << 20};
    EXPECT(!bad_overlap(IN, in_off, IN, mixed, len, 2));   // one in place, one elsewhere
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    check_inverses();
    check_statuses();
    check_verdicts();
    check_overlaps();
    const uintptr_t IN = 0x10000000, OUT = 0x4000000000, HASH = 0x70000000, SCR = 0x7800000000;
    for (int round = 0; round < 120; ++round) {
        const uint64_t count = 1 + rng() % 40;
        std::vector<uint64_t> in_off(count), in_len(count), out_off(count);
        std::vector<uint32_t> chunk_len(count), padding(count);
        uint64_t cur = 56;
        for (uint64_t o = 0; o < count; ++o) {
            const int kind = (int)(rng() % 8);
            const uint64_t spc = kind == 0 ? 1 + rng() % 4096 : kind < 4 ? 1 + rng() % 8 : 1 + rng() % 70;
            chunk_len[o] = (uint32_t)(1024 * spc);
            padding[o] = (uint32_t)(rng() % 4096);
            in_len[o] = audit::bao_len(8192 * spc);
            in_off[o] = out_off[o] = cur;
            cur += up(in_len[o], 256) + 8 * (rng() % 3);
        }
        // the scratch length: monotone in nrepair, clamped at count
        const uint64_t one = scratch_len(in_len.data(), count, 1), all = scratch_len(in_len.data(), count, count);
        EXPECT(scratch_len(in_len.data(), count, 0) == one && scratch_len(in_len.data(), count, count + 7) == all);
        uint64_t prev = one;
        for (uint64_t r = 2; r <= count; ++r) {
            const uint64_t x = scratch_len(in_len.data(), count, r);
            EXPECT(x >= prev && x % 16 == 0);
            prev = x;
        }
        EXPECT(prev == all);
        // the checks accept the call, and refuse it one byte of scratch short
        std::vector<uint64_t> n;
        int32_t status_dummy = 0;
        EXPECT(check_args(true, IN, in_off.data(), in_len.data(), count, HASH, padding.data(), chunk_len.data(), OUT,
                          out_off.data(), &status_dummy, SCR, one, &n) == CHIP_OK);
        EXPECT(check_args(true, IN, in_off.data(), in_len.data(), count, HASH, padding.data(), chunk_len.data(), OUT,
                          out_off.data(), &status_dummy, SCR, one - 1, &n) == CHIP_ERR_INVALID_ARG);
        EXPECT(n.size() == count);
        for (uint64_t o = 0; o < count; ++o) EXPECT(n[o] == 8ull * chunk_len[o]);
        // the verdict requests: 8 per stream, each shard's chunks, all tables inside the verdict part
        const VerdictLayout V(count);
        std::vector<uint32_t> spoiled = chunk_len;
        const uint64_t odd = rng() % count;
        spoiled[odd] = rng() % 2 ? 0 : chunk_len[odd] + 1024;
        audit::Plan ap;
        std::vector<uint32_t> first;
        EXPECT(plan_verdicts(IN, in_off.data(), n, spoiled.data(), HASH, &ap, &first) == CHIP_OK);
        EXPECT(first.size() == count + 1 && ap.nreq == 8 * (count - 1) && first[count] == ap.nreq);
        EXPECT(ap.table.size() + 16 == ap.lay.total && ap.lay.total <= V.first);
        for (uint64_t o = 0; o < count; ++o) {
            EXPECT(first[o + 1] - first[o] == (o == odd ? 0u : 8u));
            for (uint32_t i = 0; o != odd && i < 8; ++i) {
                const audit::Req &q = ap.reqs()[first[o] + i];
                const uint64_t spc = chunk_len[o] / 1024;
                EXPECT(q.src == IN + in_off[o] && q.hash == HASH + 32 * o && q.n == n[o] && q.N == 8 * spc);
                EXPECT(q.first == i * spc && q.last == (i + 1) * spc && q.olen == 0);
            }
        }
        uint64_t all_chunks = 0;
        for (uint64_t o = 0; o < count; ++o) all_chunks += o == odd ? 0 : n[o] / 1024;
        EXPECT(ap.total_units == 0 && ap.total_chunks == all_chunks);  // every chunk of a stream in one shard
        expect_disjoint({{V.audit, V.audit + ap.lay.total}, {V.first, V.first + 4 * (count + 1)},
                         {V.rstat, V.rstat + 32 * count}, {V.masks, V.masks + 4 * count}}, V.end);
        // the shift case of the checks and the verdict requests: offsets moved by D, and the bases moved by D
        for (const uint64_t D : plan_shift::SHIFTS) {
            const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D), out_far = plan_shift::moved(out_off, D);
            std::vector<uint64_t> n2;
            EXPECT(check_args(true, IN, in_far.data(), in_len.data(), count, HASH, padding.data(), chunk_len.data(), OUT,
                              out_far.data(), &status_dummy, SCR, one, &n2) == CHIP_OK && n2 == n);
            EXPECT(check_args(true, IN + D, in_off.data(), in_len.data(), count, HASH, padding.data(), chunk_len.data(),
                              OUT + D, out_off.data(), &status_dummy, SCR, one, &n2) == CHIP_OK && n2 == n);
            EXPECT(check_args(true, IN, in_far.data(), in_len.data(), count, HASH, padding.data(), chunk_len.data(), IN,
                              in_far.data(), &status_dummy, SCR, one, &n2) == CHIP_OK);  // in place, far
            EXPECT(!bad_overlap(IN, in_far.data(), OUT, out_far.data(), in_len.data(), count));
            EXPECT(!bad_overlap(IN, in_far.data(), IN, in_far.data(), in_len.data(), count));
            if (count >= 2) {
                std::vector<uint64_t> lap = out_far;
                lap[1] = lap[0] + 8;  // two outputs share bytes
                EXPECT(bad_overlap(IN, in_far.data(), OUT, lap.data(), in_len.data(), count));
                EXPECT(bad_overlap(IN + D, in_off.data(), IN, lap.data(), in_len.data(), count) ==
                       bad_overlap(IN, in_far.data(), IN, lap.data(), in_len.data(), count));
            }
            audit::Plan by_off, by_base;
            std::vector<uint32_t> f2, f3;
            EXPECT(plan_verdicts(IN, in_far.data(), n, spoiled.data(), HASH, &by_off, &f2) == CHIP_OK);
            EXPECT(plan_verdicts(IN + D, in_off.data(), n, spoiled.data(), HASH, &by_base, &f3) == CHIP_OK);
            EXPECT(f2 == first && f3 == first && by_off.table == by_base.table && by_off.total_chunks == ap.total_chunks);
            EXPECT(plan_shift::shifted_words(ap.table, by_off.table, D) == (long)ap.nreq);  // each request's stream address
            for (uint64_t r = 0; r < ap.nreq; ++r)
                EXPECT(by_off.reqs()[r].src == ap.reqs()[r].src + D && by_off.reqs()[r].hash == ap.reqs()[r].hash);
        }
        // some streams to repair, each with a random 4-subset; packed into passes under several scratch sizes
        std::vector<Repair> reps;
        for (uint64_t o = 0; o < count; ++o) {
            if (rng() % 3 == 0) continue;
            Repair r{o, n[o], padding[o], {}};
            uint32_t m = 0;
            while (__builtin_popcount(m) != 4) m = (uint32_t)(rng() % 256);
            uint32_t k = 0;
            for (uint32_t i = 0; i < 8; ++i)
                if (m >> i & 1) r.sel[k++] = (uint8_t)i;
            reps.push_back(r);
        }
        const uint64_t some = scratch_len(in_len.data(), count, 1 + rng() % count);
        for (const uint64_t given : {one, some, all, all + 4096}) {
            const uint64_t avail = given - V.end;
            const auto passes = pack(reps, avail);
            if (given >= all) EXPECT(passes.size() == (reps.empty() ? 0u : 1u));
            size_t next = 0;
            for (const auto &range : passes) {  // every repair exactly once, in order
                EXPECT(range.first == next && range.second > range.first);
                next = range.second;
                const uint64_t R = range.second - range.first;
                Pass p;
                EXPECT(plan_pass(reps.data() + range.first, R, SCR + V.end, IN, in_off.data(), OUT, out_off.data(), HASH,
                                 &p) == CHIP_OK);
                EXPECT(p.lay.total <= avail && p.table.size() == p.lay.table_end && p.R == R);
                std::vector<Region> regs = {{p.lay.recs, p.lay.recs + 64 * R},
                                            {p.lay.commits, p.lay.commits + 64 * R},
                                            {p.lay.blocks, p.lay.blocks + 4 * (R + 1)},
                                            {p.lay.units, p.lay.units + 8 * (R + 1)},
                                            {p.lay.ok, p.lay.ok + 4 * R},
                                            {p.lay.h2, p.lay.h2 + 32 * R},
                                            {p.lay.renc, p.lay.renc + p.enc.lay.total}};
                EXPECT(p.blocks()[0] == 0 && p.units()[0] == 0);
                EXPECT(p.blocks()[R] == p.total_blocks && p.units()[R] == p.total_units);
                EXPECT(p.enc.count == R && p.enc.total_blocks == p.total_blocks);
                for (uint64_t j = 0; j < R; ++j) {
                    const Repair &r = reps[range.first + j];
                    const Rec &a = p.recs()[j];
                    const Commit &k = p.commits()[j];
                    const uint64_t base = SCR + V.end;
                    EXPECT(a.src == IN + in_off[r.obj] && a.C == r.n / 8 && a.N == r.n / 1024 && a.dst % 16 == 0);
                    EXPECT(p.blocks()[j + 1] - p.blocks()[j] == (a.C + 4095) / 4096);
                    EXPECT(k.len == in_len[r.obj] && k.out == OUT + out_off[r.obj] && k.want == HASH + 32 * r.obj);
                    EXPECT(k.row % 8 == 0 && k.got == base + p.lay.h2 + 32 * j);
                    EXPECT(p.units()[j + 1] - p.units()[j] == (k.len + 15) / 16);
                    regs.push_back({a.dst - base, a.dst - base + 4 * a.C});
                    regs.push_back({k.row - base, k.row - base + k.len});
                    const ragged::Obj &e = p.enc.objs()[j];  // the re-encode reads the primaries, writes the row
                    EXPECT((uintptr_t)e.src == a.dst && (uintptr_t)e.stream == k.row && e.C == a.C && e.N == a.N);
                    EXPECT(e.valid == 4 * a.C - r.pad);
                }
                expect_disjoint(regs, p.lay.total);
                // the shift case of a pass: the streams read and the outputs committed D higher, the scratch where it was
                for (const uint64_t D : plan_shift::SHIFTS) {
                    const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D), out_far = plan_shift::moved(out_off, D);
                    Pass by_off, by_base;
                    EXPECT(plan_pass(reps.data() + range.first, R, SCR + V.end, IN, in_far.data(), OUT, out_far.data(), HASH,
                                     &by_off) == CHIP_OK);
                    EXPECT(plan_pass(reps.data() + range.first, R, SCR + V.end, IN + D, in_off.data(), OUT + D, out_off.data(),
                                     HASH, &by_base) == CHIP_OK);
                    EXPECT(by_off.table == by_base.table && by_off.enc.table == by_base.enc.table);
                    EXPECT(by_off.total_blocks == p.total_blocks && by_off.total_units == p.total_units);
                    EXPECT(by_off.enc.table == p.enc.table);  // the re-encode works inside the scratch
                    EXPECT(plan_shift::shifted_words(p.table, by_off.table, D) == (long)(2 * R));
                    for (uint64_t j = 0; j < R; ++j) {
                        EXPECT(by_off.recs()[j].src == p.recs()[j].src + D && by_off.recs()[j].dst == p.recs()[j].dst);
                        EXPECT(by_off.commits()[j].out == p.commits()[j].out + D && by_off.commits()[j].row == p.commits()[j].row);
                    }
                }
            }
            EXPECT(next == reps.size());
        }
    }
    // call-level refusals
    {
        std::vector<uint64_t> n;
        int32_t st = 0;
        const uint64_t len[2] = {audit::bao_len(8192), audit::bao_len(8192 * 5)}, off[2] = {56, 65536 + 8};
        const uint32_t cl[2] = {1024, 5120}, pad[2] = {1, 2};
        const uint64_t need = scratch_len(len, 2, 1);
        auto call = [&](uintptr_t in, const uint64_t *io, const uint64_t *il, uintptr_t hash, uintptr_t out,
                        const uint64_t *oo, uintptr_t scr, uint64_t sl) {
            return check_args(true, in, io, il, 2, hash, pad, cl, out, oo, &st, scr, sl, &n);
        };
        EXPECT(call(IN, off, len, HASH, OUT, off, SCR, need) == CHIP_OK);
        EXPECT(call(IN, off, len, HASH, IN, off, SCR, need) == CHIP_OK);  // in place
        EXPECT(call(0, off, len, HASH, OUT, off, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off, len, HASH, OUT, off, SCR + 8, need) == CHIP_ERR_INVALID_ARG);
        const uint64_t off4[2] = {60, 65536 + 8};
        EXPECT(call(IN, off4, len, HASH, OUT, off, SCR, need) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off, len, HASH, OUT, off4, SCR, need) == CHIP_ERR_INVALID_ARG);
        const uint64_t big[2] = {len[0], audit::bao_len(MAX_CONTENT + 8192)};
        EXPECT(call(IN, off, big, HASH, OUT, off, SCR, ~0ull) == CHIP_ERR_INVALID_ARG);
        const uint64_t gap[2] = {len[0] + 8, len[1]};
        EXPECT(call(IN, off, gap, HASH, OUT, off, SCR, need) == CHIP_ERR_BAO_TRUNCATED);
        EXPECT(call(IN, off, gap, 0, OUT, off, SCR, need) == CHIP_ERR_BAO_TRUNCATED);
        EXPECT(call(IN, off, gap, HASH, OUT, off, SCR, 0) == CHIP_ERR_INVALID_ARG);
        EXPECT(call(IN, off, len, 0, OUT, off, SCR, need) == CHIP_ERR_HASH_DECODE);
        EXPECT(check_args(true, IN, off, len, 1ull << 31, HASH, pad, cl, OUT, off, &st, SCR, ~0ull, &n) ==
               CHIP_ERR_INVALID_ARG);
        EXPECT(check_args(true, 0, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, &n) == CHIP_OK);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
