// repair_plan.hpp — host side of the ragged scrub (include/carbonado_hip_repair.h):
// argument checks, the scratch layout, the verdict requests (8 slice requests
// per stream through audit_plan.hpp), the per-object statuses scrub decides
// from a mask, the packing of the streams to repair into passes, and the
// tables the kernels of repair_kernels.hip are driven by (the nested re-encode
// is ragged_plan.hpp's).  Pure host code without a HIP type in it, so a
// stand-alone program can exercise it under a sanitizer
// (tests/repair_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/carbonado_hip_repair.h"
#include "audit_plan.hpp"
#include "gf256.hpp"
#include "ragged_plan.hpp"

namespace chip {
namespace repair {

constexpr uint64_t MAX_CONTENT = 2 * ragged::MAX_OBJECT;  // bao content of a stream: the 8 shards of a 16 MiB object
constexpr uint64_t BLOCK = 4096;       // bytes of every selected share per workgroup of the decode kernel
constexpr uint64_t UNIT = 16;          // bytes per work item of the commit gather
constexpr uint64_t ROW_OFFSET = 56;    // a staged row's stream: every chunk and node on a 64-B boundary
constexpr uint32_t K = 4, M = 8;

using rules::up;

// One stream to repair, as repair_decode_kernel reads it (device scratch).
struct Rec {
    uint64_t src;      // address of the damaged stream
    uint64_t dst;      // address of the 4 primaries, C bytes each, contiguous (16-B aligned)
    uint64_t C;        // shard length
    uint32_t N;        // chunks of the stream (8 C / 1024)
    uint8_t sel[4];    // the selected shares' true indices
    uint8_t coef[16];  // inverse of those rows of the encoding matrix: primary r = sum_s coef[4 r + s] * share sel[s]
    uint64_t pad_[2];
};
static_assert(sizeof(Rec) == 64, "record layout");

// The same stream, as the hash compare and the commit gather read it.
struct Commit {
    uint64_t row;   // address of the staged re-encoded stream
    uint64_t out;   // address of the object's output range
    uint64_t len;   // bytes of the stream (a multiple of 8)
    uint64_t want;  // address of the expected hash
    uint64_t got;   // address of the re-encoded stream's hash
    uint64_t pad_[3];
};
static_assert(sizeof(Commit) == 64, "record layout");

// ---- the scratch ---------------------------------------------------------------
// [verdict part | pass part], every region on a 256-B boundary of the scratch.
// Verdict part: [audit table of 8 count requests | first request per object |
// request status words | masks].
struct VerdictLayout {
    uint64_t audit = 0, first = 0, rstat = 0, masks = 0, end = 0;
    explicit VerdictLayout(uint64_t count) {
        first = up(audit::ScratchLayout(8 * count).total, 256);
        rstat = first + up((count + 1) * 4, 256);
        masks = rstat + up(8 * count * 4, 256);
        end = masks + up(count * 4, 256);
    }
};

// What one stream of content n (= 8 C) adds to a pass.
struct Cost {
    uint64_t prim = 0, row = 0, groups = 0;
};
inline Cost cost_of(uint64_t n) {
    Cost c;
    c.prim = up(n / 2, 256);
    c.row = up(ROW_OFFSET + audit::bao_len(n), 256);
    c.groups = ragged::groups_of(CHIP_FORMAT_BAO | CHIP_FORMAT_ZFEC, n);
    return c;
}

// Pass part, relative to VerdictLayout::end: [records | commit records |
// blocks prefix | units prefix] (the uploaded table), then [verdict per repair |
// re-encoded hashes | decoded primaries | staged rows | nested ragged-encode
// scratch].  Its size depends on the number of repairs and the sums of their
// costs only, not on their order.
struct PassLayout {
    uint64_t recs = 0, commits = 0, blocks = 0, units = 0, table_end = 0, ok = 0, h2 = 0, prim = 0, rows = 0, renc = 0,
             total = 0;
    PassLayout(uint64_t R, const Cost &sum) {
        commits = up(R * sizeof(Rec), 256);
        blocks = commits + up(R * sizeof(Commit), 256);
        units = blocks + up((R + 1) * 4, 256);
        table_end = units + up((R + 1) * 8, 256);
        ok = table_end;
        h2 = ok + up(R * 4, 256);
        prim = h2 + up(R * 32, 256);
        rows = prim + sum.prim;
        renc = rows + sum.row;
        total = renc + up(ragged::ScratchLayout(R, sum.groups).total, 16);
    }
};

// content of a stream a call could repair (0: never repaired, costs nothing)
inline uint64_t repairable_content(uint64_t in_len) {
    uint64_t n = 0;
    if (!audit::bao_content(in_len, &n) || n == 0 || n > MAX_CONTENT || n % (8 * 1024)) return 0;
    return n;
}

inline uint64_t scratch_len(const uint64_t *in_len, uint64_t count, uint64_t nrepair) {
    if (count >= (1ull << 31)) count = 0;
    const uint64_t R = std::max<uint64_t>(1, std::min(nrepair, count));
    std::vector<uint64_t> n;
    n.reserve(count);
    for (uint64_t o = 0; in_len && o < count; ++o) n.push_back(repairable_content(in_len[o]));
    const uint64_t top = std::min<uint64_t>(R, n.size());
    std::partial_sort(n.begin(), n.begin() + top, n.end(), std::greater<uint64_t>());
    Cost sum;
    for (uint64_t j = 0; j < top; ++j) {
        if (!n[j]) break;
        const Cost c = cost_of(n[j]);
        sum.prim += c.prim; sum.row += c.row; sum.groups += c.groups;
    }
    return VerdictLayout(count).end + PassLayout(R, sum).total;
}

// ---- argument checks -----------------------------------------------------------
struct Range {
    uint64_t lo, hi, obj;
};

// true when an output range meets another output range, or any input range
// other than its own object's identical range
inline bool bad_overlap(uintptr_t d_in, const uint64_t *in_off, uintptr_t d_out, const uint64_t *out_off,
                        const uint64_t *in_len, uint64_t count) {
    std::vector<Range> outs;
    outs.reserve(count);
    for (uint64_t o = 0; o < count; ++o)
        if (in_len[o]) outs.push_back({d_out + out_off[o], d_out + out_off[o] + in_len[o], o});
    std::sort(outs.begin(), outs.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < outs.size(); ++i)
        if (outs[i - 1].hi > outs[i].lo) return true;
    for (uint64_t o = 0; o < count; ++o) {  // the outputs are disjoint and sorted: those meeting an input are neighbours
        if (!in_len[o]) continue;
        const uint64_t lo = d_in + in_off[o], hi = lo + in_len[o];
        auto it = std::upper_bound(outs.begin(), outs.end(), lo, [](uint64_t x, const Range &r) { return x < r.hi; });
        for (; it != outs.end() && it->lo < hi; ++it)
            if (!(it->obj == o && it->lo == lo && it->hi == hi)) return true;
    }
    return false;
}

// The checks both calls share, in the header's order; n[o] = each stream's
// content length.  `scrub`: the output side is checked too.
inline int check_args(bool scrub, uintptr_t d_in, const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                      uintptr_t d_hash, const uint32_t *padding, const uint32_t *chunk_len, uintptr_t d_out,
                      const uint64_t *out_off, const void *result, uintptr_t d_scratch, uint64_t scratch_len_given,
                      std::vector<uint64_t> *n) {
    if (count == 0) return CHIP_OK;
    if (!d_in || !in_off || !in_len || !chunk_len || !result || !d_scratch) return CHIP_ERR_INVALID_ARG;
    if (scrub && (!padding || !d_out || !out_off)) return CHIP_ERR_INVALID_ARG;
    if (count >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    if (d_scratch % 16) return CHIP_ERR_INVALID_ARG;
    bool truncated = false;
    n->assign(count, 0);
    for (uint64_t o = 0; o < count; ++o) {
        if ((d_in + in_off[o]) % 8 || (scrub && (d_out + out_off[o]) % 8)) return CHIP_ERR_INVALID_ARG;
        if (!audit::bao_content(in_len[o], &(*n)[o])) truncated = true;
        else if ((*n)[o] > MAX_CONTENT) return CHIP_ERR_INVALID_ARG;
    }
    if (scrub && bad_overlap(d_in, in_off, d_out, out_off, in_len, count)) return CHIP_ERR_INVALID_ARG;
    if (scratch_len_given < scratch_len(in_len, count, 1)) return CHIP_ERR_INVALID_ARG;
    if (truncated) return CHIP_ERR_BAO_TRUNCATED;
    return d_hash ? CHIP_OK : CHIP_ERR_HASH_DECODE;
}

// ---- verdicts --------------------------------------------------------------------
// shard length of stream o when chunk_len[o] fits its content, else 0 (mask 0, status 7)
inline uint64_t shard_len_of(uint64_t n, uint32_t chunk_len) {
    const uint64_t C = chunk_len;
    return (C == 0 || C % 1024 || n != M * C) ? 0 : C;
}

// 8 slice requests (index = i spc, count = spc, no content) per stream whose
// chunk_len fits; first[o] = its first request, first[count] = their number.
inline int plan_verdicts(uintptr_t d_in, const uint64_t *in_off, const std::vector<uint64_t> &n,
                         const uint32_t *chunk_len, uintptr_t d_hash, audit::Plan *p, std::vector<uint32_t> *first) {
    const uint64_t count = n.size();
    first->assign(count + 1, 0);
    uint64_t nreq = 0;
    for (uint64_t o = 0; o < count; ++o) {
        (*first)[o] = (uint32_t)nreq;
        if (shard_len_of(n[o], chunk_len[o])) nreq += M;
    }
    (*first)[count] = (uint32_t)nreq;
    audit::start(p, nreq);
    for (uint64_t o = 0; o < count; ++o) {
        const uint64_t spc = shard_len_of(n[o], chunk_len[o]) / 1024;
        for (uint64_t i = 0; spc && i < M; ++i) {
            audit::Sel s = audit::select(n[o], i * spc, spc);
            s.olen = 0;
            audit::put(p, (*first)[o] + i, s, n[o], d_in + in_off[o], 0, d_hash + 32 * o, 0);
        }
    }
    return audit::finish(p);
}

// What scrub decides for a stream from its mask before any repair work
// (chip_scrub_batch_dev's order): a status, or rules::REPAIR.
inline int pre_status(uint64_t in_len, uint64_t n, uint32_t chunk_len, uint32_t padding, uint32_t mask) {
    const uint64_t C = shard_len_of(n, chunk_len);
    if (!C) return CHIP_ERR_ZFEC;
    const int good = __builtin_popcount(mask & 0xFFu);
    if (good == (int)M) return CHIP_ERR_UNNECESSARY_SCRUB;  // decoding.rs:169-170
    return rules::scrub_verdict(in_len, C, padding, (uint32_t)good);
}

// the 16 coefficients of a record: the inverse of rows sel[0..4) of zfec_enc_matrix(4, 8)
inline bool inverse_for(const uint8_t sel[4], uint8_t coef[16]) {
    static const std::vector<uint8_t> enc = zfec_enc_matrix(K, M);
    std::vector<uint8_t> a(K * K);
    for (uint32_t s = 0; s < K; ++s) {
        if (sel[s] >= M) return false;
        std::memcpy(&a[s * K], &enc[sel[s] * K], K);
    }
    if (!gf_invert(a, K)) return false;
    std::memcpy(coef, a.data(), K * K);
    return true;
}

// ---- passes ------------------------------------------------------------------------
struct Repair {
    uint64_t obj;    // the object
    uint64_t n;      // its content (8 C)
    uint32_t pad;    // its padding
    uint8_t sel[4];  // the shares to decode from
};

// [begin, end) of `reps` per pass: as many, in order, as fit `avail` bytes
inline std::vector<std::pair<size_t, size_t>> pack(const std::vector<Repair> &reps, uint64_t avail) {
    std::vector<std::pair<size_t, size_t>> out;
    size_t b = 0;
    Cost sum;
    for (size_t j = 0; j < reps.size(); ++j) {
        const Cost c = cost_of(reps[j].n);
        Cost with = sum;
        with.prim += c.prim; with.row += c.row; with.groups += c.groups;
        if (j > b && PassLayout(j + 1 - b, with).total > avail) {
            out.emplace_back(b, j);
            b = j;
            with = c;
        }
        sum = with;
    }
    if (b < reps.size()) out.emplace_back(b, reps.size());
    return out;
}

// The tables of one pass and its nested re-encode.
struct Pass {
    std::vector<uint8_t> table;  // [records | commit records | blocks prefix | units prefix], as uploaded
    PassLayout lay{0, Cost{}};
    uint64_t R = 0, total_blocks = 0, total_units = 0;
    ragged::Plan enc;            // encode() at Zfec|Bao of the decoded primaries into the staged rows
    Rec *recs() { return reinterpret_cast<Rec *>(table.data()); }
    Commit *commits() { return reinterpret_cast<Commit *>(table.data() + lay.commits); }
    uint32_t *blocks() { return reinterpret_cast<uint32_t *>(table.data() + lay.blocks); }
    uint64_t *units() { return reinterpret_cast<uint64_t *>(table.data() + lay.units); }
};

// `base` = address of the pass part of the scratch (d_scratch + VerdictLayout::end)
inline int plan_pass(const Repair *reps, uint64_t R, uintptr_t base, uintptr_t d_in, const uint64_t *in_off,
                     uintptr_t d_out, const uint64_t *out_off, uintptr_t d_hash, Pass *p) {
    Cost sum;
    for (uint64_t j = 0; j < R; ++j) {
        const Cost c = cost_of(reps[j].n);
        sum.prim += c.prim; sum.row += c.row; sum.groups += c.groups;
    }
    p->R = R;
    p->lay = PassLayout(R, sum);
    p->table.assign(p->lay.table_end, 0);
    std::vector<uint64_t> eoff(R), en(R), roff(R), rlen(R);
    uint64_t prim = p->lay.prim, row = p->lay.rows, b = 0, u = 0;
    for (uint64_t j = 0; j < R; ++j) {
        const Repair &r = reps[j];
        const Cost c = cost_of(r.n);
        const uint64_t C = r.n / M, len = audit::bao_len(r.n);
        Rec &a = p->recs()[j];
        a.src = d_in + in_off[r.obj];
        a.dst = base + prim;
        a.C = C;
        a.N = (uint32_t)(r.n / 1024);
        std::memcpy(a.sel, r.sel, K);
        if (!inverse_for(r.sel, a.coef)) return CHIP_ERR_ZFEC;
        Commit &k = p->commits()[j];
        k.row = base + row + ROW_OFFSET;
        k.out = d_out + out_off[r.obj];
        k.len = len;
        k.want = d_hash + 32 * r.obj;
        k.got = base + p->lay.h2 + 32 * j;
        p->blocks()[j] = (uint32_t)b;
        p->units()[j] = u;
        b += (C + BLOCK - 1) / BLOCK;
        u += (len + UNIT - 1) / UNIT;
        if (b >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
        eoff[j] = prim; en[j] = K * C - r.pad; roff[j] = row + ROW_OFFSET;
        prim += c.prim;
        row += c.row;
    }
    p->blocks()[R] = (uint32_t)b;
    p->units()[R] = u;
    p->total_blocks = b;
    p->total_units = u;
    const int st = ragged::plan_encode(CHIP_FORMAT_BAO | CHIP_FORMAT_ZFEC, base, eoff.data(), en.data(), R, base,
                                       roff.data(), rlen.data(), &p->enc);
    if (st != CHIP_OK) return st;
    for (uint64_t j = 0; j < R; ++j)
        if (rlen[j] != p->commits()[j].len) return CHIP_ERR_INVALID_ARG;  // (pre_status made sure of it)
    return CHIP_OK;
}

}  // namespace repair
}  // namespace chip
