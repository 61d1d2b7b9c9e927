// ragged_plan_check.cpp — the host logic of the ragged batches
// (carbonado_amd/csrc/ragged_plan.hpp: layout, argument checks, descriptor and
// prefix tables, overlap detection) driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_ragged_cpu.py).  No device: the
// addresses are made-up integers, nothing is dereferenced.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../carbonado_amd/csrc/ragged_plan.hpp"
#include "plan_shift.hpp"

using namespace chip::ragged;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

// the invariants the kernels rely on, whatever the mix of lengths
static void check_plan(Plan &p, uint8_t format) {
    const uint64_t count = p.count;
    EXPECT(p.table.size() == p.lay.gcv);
    EXPECT(p.groups()[0] == 0 && p.blocks()[0] == 0);
    EXPECT(p.groups()[count] == p.total_groups && p.blocks()[count] == p.total_blocks);
    for (uint64_t o = 0; o < count; ++o) {
        const Obj &a = p.objs()[o];
        EXPECT(p.groups()[o] <= p.groups()[o + 1] && p.blocks()[o] <= p.blocks()[o + 1]);
        EXPECT(a.g0 == p.groups()[o]);
        EXPECT(a.N == chunks(a.n) && a.N <= GROUP * TOP_MAX_G);
        if (format & CHIP_FORMAT_BAO) EXPECT(p.groups()[o + 1] - p.groups()[o] == (a.N + GROUP - 1) / GROUP);
        else EXPECT(p.groups()[o + 1] == 0);
    }
    EXPECT(p.lay.total >= p.lay.gcv + 32 * p.total_groups);
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 0) : 1u;
    std::mt19937_64 rng(seed);
    const uintptr_t IN = 0x10000000, OUT = 0x80000000;
    for (int round = 0; round < 200; ++round) {
        static const uint8_t FORMATS[3] = {4, 8, 12};
        const uint8_t format = FORMATS[rng() % 3];
        const uint64_t count = rng() % 40;
        std::vector<uint64_t> n(count), in_off(count), out_off(count), out_len(count), lay_len(count);
        uint64_t cur = 0;
        for (uint64_t o = 0; o < count; ++o) {
            const int kind = (int)(rng() % 4);
            n[o] = kind == 0 ? rng() % 70 : kind == 1 ? rng() % 70000 : kind == 2 ? rng() % (MAX_OBJECT + 1)
                                                                                 : 1024 * (rng() % 300);
            in_off[o] = cur;
            cur += up(n[o], 16) + 16;
        }
        uint64_t total = 0;
        const uint64_t so = 8 * (rng() % 32);
        EXPECT(layout(format, n.data(), count, 256, so, out_off.data(), lay_len.data(), &total) == CHIP_OK);
        for (uint64_t o = 0; o < count; ++o) EXPECT(out_off[o] + lay_len[o] <= total);
        EXPECT(!ranges_overlap(out_off.data(), lay_len.data(), count));
        Plan p;
        EXPECT(plan_encode(format, IN, in_off.data(), n.data(), count, OUT, out_off.data(), out_len.data(), &p) == CHIP_OK);
        EXPECT(out_len == lay_len);
        check_plan(p, format);
        EXPECT(scratch_len(format, n.data(), count, 0) == p.lay.total);
        // decode of those encodings, outputs packed like the inputs
        std::vector<uint32_t> pad(count);
        std::vector<uint64_t> dec_len(count);
        for (uint64_t o = 0; o < count; ++o) pad[o] = (format & CHIP_FORMAT_ZFEC) ? (uint32_t)(4 * shard_len(n[o]) - n[o]) : 0;
        Plan d;
        EXPECT(plan_decode(format, OUT, out_off.data(), out_len.data(), count, pad.data(), IN, in_off.data(),
                           dec_len.data(), &d) == CHIP_OK);
        EXPECT(dec_len == n);
        check_plan(d, format);
        EXPECT(scratch_len(format, out_len.data(), count, 1) == d.lay.total);
        // the shift case: every offset moved by D, and the bases moved by D: the same tables, the addresses D higher
        for (const uint64_t D : plan_shift::SHIFTS) {
            const std::vector<uint64_t> in_far = plan_shift::moved(in_off, D), out_far = plan_shift::moved(out_off, D);
            std::vector<uint64_t> len2(count), len3(count);
            EXPECT(!ranges_overlap(out_far.data(), lay_len.data(), count));
            for (int decode = 0; decode < 2; ++decode) {
                Plan &first = decode ? d : p;
                Plan by_off, by_base;
                if (decode) {
                    EXPECT(plan_decode(format, OUT, out_far.data(), out_len.data(), count, pad.data(), IN, in_far.data(),
                                       len2.data(), &by_off) == CHIP_OK);
                    EXPECT(plan_decode(format, OUT + D, out_off.data(), out_len.data(), count, pad.data(), IN + D,
                                       in_off.data(), len3.data(), &by_base) == CHIP_OK);
                    EXPECT(len2 == n && len3 == n);
                } else {
                    EXPECT(plan_encode(format, IN, in_far.data(), n.data(), count, OUT, out_far.data(), len2.data(),
                                       &by_off) == CHIP_OK);
                    EXPECT(plan_encode(format, IN + D, in_off.data(), n.data(), count, OUT + D, out_off.data(), len3.data(),
                                       &by_base) == CHIP_OK);
                    EXPECT(len2 == lay_len && len3 == lay_len);
                }
                EXPECT(by_off.table == by_base.table && by_off.lay.total == first.lay.total);
                EXPECT(by_off.total_groups == first.total_groups && by_off.total_blocks == first.total_blocks);
                // per object: two addresses (src and stream, or stream and out) D higher, nothing else changed
                EXPECT(plan_shift::shifted_words(first.table, by_off.table, D) == (long)(2 * count));
                for (uint64_t o = 0; o < count; ++o) {
                    const Obj &a = first.objs()[o], &b = by_off.objs()[o];
                    EXPECT((uintptr_t)b.stream == (uintptr_t)a.stream + D);
                    EXPECT((uintptr_t)(decode ? b.out : b.src) == (uintptr_t)(decode ? a.out : a.src) + D);
                }
            }
            if (count >= 2 && out_len[0] && out_len[1]) {  // an overlap is an overlap at any height
                std::vector<uint64_t> bad = out_far;
                bad[1] = bad[0];
                EXPECT(ranges_overlap(bad.data(), out_len.data(), count));
            }
        }
        if (count >= 2) {  // two outputs made to share a byte; a misaligned one; an oversize one
            std::vector<uint64_t> bad = out_off;
            const uint64_t a = rng() % count, b = (a + 1) % count;
            if (out_len[a] && out_len[b]) {
                bad[b] = bad[a];
                EXPECT(plan_encode(format, IN, in_off.data(), n.data(), count, OUT, bad.data(), out_len.data(), &p) ==
                       CHIP_ERR_INVALID_ARG);
            }
            bad = out_off;
            bad[a] += 4;
            EXPECT(plan_encode(format, IN, in_off.data(), n.data(), count, OUT, bad.data(), out_len.data(), &p) ==
                   CHIP_ERR_INVALID_ARG);
            std::vector<uint64_t> big = n;
            big[a] = MAX_OBJECT + 1 + rng() % 100;
            EXPECT(plan_encode(format, IN, in_off.data(), big.data(), count, OUT, out_off.data(), out_len.data(), &p) ==
                   CHIP_ERR_INVALID_ARG);
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
