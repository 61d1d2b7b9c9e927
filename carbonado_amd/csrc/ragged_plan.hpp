// ragged_plan.hpp — host side of the ragged batches (include/carbonado_hip_ext.h):
// argument checks, the per-object descriptor table the kernels of
// ragged_kernels.hip are driven by, the scratch layout and the caller's
// output layout.  Pure host code without a HIP type in it, so a stand-alone
// program can exercise it under a sanitizer (tests/ragged_plan_check.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/carbonado_hip_ext.h"
#include "stream_rules.hpp"

namespace chip {
namespace ragged {

using rules::bao_content;
using rules::bao_len;
using rules::chunks;
using rules::ranges_overlap;
using rules::up;

constexpr uint64_t MAX_OBJECT = uint64_t(16) << 20;  // per object; its Zfec|Bao stream is KM_MAX_N chunks
constexpr uint64_t GROUP = 64;                      // chunks per workgroup of the group kernel
constexpr uint64_t PARITY_BLOCK = 4096;             // bytes of every shard per workgroup of the parity kernel
constexpr uint64_t COPY_BLOCK = 16384;              // bytes per workgroup of the copy kernel (Zfec-only decode)
constexpr uint64_t TOP_MAX_G = 2 * MAX_OBJECT / 1024 / GROUP;  // groups the top kernel holds in LDS (512)

// One object of a call, as the kernels read it (device scratch).
struct Obj {
    const uint8_t *src;  // encode: the input (zero past `valid`)
    uint8_t *stream;     // Bao bit: the object's stream (encode: written, decode: read); Zfec only: its 8 shards
    uint8_t *out;        // decode: the content
    uint64_t valid;      // encode: input bytes
    uint64_t C;          // zfec shard length, 0 without the Zfec bit
    uint64_t n;          // bao content bytes
    uint64_t out_limit;  // decode: content bytes written
    uint32_t N;          // chunks of the bao content
    uint32_t g0;         // its first group (= groups[o] of the prefix array)
};
static_assert(sizeof(Obj) == 64, "descriptor layout");

inline uint64_t shard_len(uint64_t n) { return (n + 4095) / 4096 * 1024; }  // utils.rs:47-58 at k = 4

inline bool device_format(uint8_t f) {
    return f == CHIP_FORMAT_BAO || f == CHIP_FORMAT_ZFEC || f == (CHIP_FORMAT_BAO | CHIP_FORMAT_ZFEC);
}

inline uint64_t encoded_len(uint8_t format, uint64_t n) {
    const uint64_t z = (format & CHIP_FORMAT_ZFEC) ? 8 * shard_len(n) : n;
    return (format & CHIP_FORMAT_BAO) ? bao_len(z) : z;
}

// scratch: [objs | groups prefix | blocks prefix | group CVs], each on a 256-B boundary
struct ScratchLayout {
    uint64_t objs = 0, groups = 0, blocks = 0, gcv = 0, total = 0;
    ScratchLayout(uint64_t count, uint64_t total_groups) {
        groups = up(count * sizeof(Obj), 256);
        blocks = groups + up((count + 1) * 4, 256);
        gcv = blocks + up((count + 1) * 4, 256);
        total = gcv + 32 * total_groups + 16;
    }
};

struct Plan {
    std::vector<uint8_t> table;  // the bytes in front of the group CVs, as uploaded
    uint64_t count = 0, total_groups = 0, total_blocks = 0;
    ScratchLayout lay{0, 0};
    Obj *objs() { return reinterpret_cast<Obj *>(table.data()); }
    uint32_t *groups() { return reinterpret_cast<uint32_t *>(table.data() + lay.groups); }
    uint32_t *blocks() { return reinterpret_cast<uint32_t *>(table.data() + lay.blocks); }
};

// groups (Bao bit) of an object whose bao content is n bytes
inline uint64_t groups_of(uint8_t format, uint64_t n) {
    return (format & CHIP_FORMAT_BAO) ? (chunks(n) + GROUP - 1) / GROUP : 0;
}

inline int layout(uint8_t format, const uint64_t *n, uint64_t count, uint64_t align, uint64_t stream_offset,
                  uint64_t *out_off, uint64_t *out_len, uint64_t *total) {
    if (!device_format(format) || !total || (count && (!n || !out_off || !out_len))) return CHIP_ERR_INVALID_ARG;
    if (align == 0 || align % 256 || stream_offset >= align || stream_offset % 8) return CHIP_ERR_INVALID_ARG;
    if (!(format & CHIP_FORMAT_BAO)) stream_offset = 0;  // shards without a stream around them: at the row's start
    uint64_t row = 0;
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > MAX_OBJECT) return CHIP_ERR_INVALID_ARG;
        out_len[o] = encoded_len(format, n[o]);
        out_off[o] = row + stream_offset;
        row += up(stream_offset + out_len[o], align);
    }
    *total = row;
    return CHIP_OK;
}

inline int finish(Plan *p) {
    uint64_t g = 0, b = 0;
    Obj *objs = p->objs();
    for (uint64_t o = 0; o < p->count; ++o) {
        const uint64_t og = p->groups()[o], ob = p->blocks()[o];  // per-object counts so far
        objs[o].g0 = (uint32_t)g;
        p->groups()[o] = (uint32_t)g;
        p->blocks()[o] = (uint32_t)b;
        g += og;
        b += ob;
        if (g >= (1ull << 31) || b >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    }
    p->groups()[p->count] = (uint32_t)g;
    p->blocks()[p->count] = (uint32_t)b;
    p->total_groups = g;
    p->total_blocks = b;
    return CHIP_OK;
}

inline void start(Plan *p, uint64_t count) {
    p->count = count;
    p->lay = ScratchLayout(count, 0);
    p->table.assign(p->lay.gcv, 0);
}

// The table of an encode call; out_len[o] = each object's encoded length.
// Addresses are plain integers here (base + offset).
inline int plan_encode(uint8_t format, uintptr_t d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                       uintptr_t d_out, const uint64_t *out_off, uint64_t *out_len, Plan *p) {
    if (format > 15 || (format & (CHIP_FORMAT_ECIES | CHIP_FORMAT_SNAPPY)) || !device_format(format))
        return CHIP_ERR_INVALID_ARG;
    if (count >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    if (count && (!in_off || !n || !out_off || !out_len)) return CHIP_ERR_INVALID_ARG;
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    start(p, count);
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > MAX_OBJECT) return CHIP_ERR_INVALID_ARG;
        const uintptr_t in = d_in + in_off[o], out = d_out + out_off[o];
        out_len[o] = encoded_len(format, n[o]);
        if ((n[o] && !d_in) || (out_len[o] && !d_out)) return CHIP_ERR_INVALID_ARG;
        if ((in % 16) || (out % (bao ? 8 : 16))) return CHIP_ERR_INVALID_ARG;
        Obj &a = p->objs()[o];
        a.src = reinterpret_cast<const uint8_t *>(in);
        a.stream = reinterpret_cast<uint8_t *>(out);
        a.valid = n[o];
        a.C = zfec ? shard_len(n[o]) : 0;
        a.n = zfec ? 8 * a.C : n[o];
        a.N = (uint32_t)chunks(a.n);
        p->groups()[o] = (uint32_t)groups_of(format, a.n);
        p->blocks()[o] = (uint32_t)((a.C + PARITY_BLOCK - 1) / PARITY_BLOCK);
    }
    if (ranges_overlap(out_off, out_len, count)) return CHIP_ERR_INVALID_ARG;
    const int st = finish(p);
    if (st != CHIP_OK) return st;
    p->lay = ScratchLayout(count, p->total_groups);
    return CHIP_OK;
}

// The table of a decode call; out_len[o] = each object's decoded length.
inline int plan_decode(uint8_t format, uintptr_t d_in, const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                       const uint32_t *padding, uintptr_t d_out, const uint64_t *out_off, uint64_t *out_len,
                       Plan *p) {
    if (format > 15 || (format & (CHIP_FORMAT_ECIES | CHIP_FORMAT_SNAPPY)) || !device_format(format))
        return CHIP_ERR_INVALID_ARG;
    if (count >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    if (count && (!in_off || !in_len || !out_off || !out_len || (zfec && !padding))) return CHIP_ERR_INVALID_ARG;
    start(p, count);
    for (uint64_t o = 0; o < count; ++o) {
        uint64_t blen = in_len[o];  // bytes entering zfec (decoding.rs:90-99)
        if (bao && !bao_content(in_len[o], &blen)) return CHIP_ERR_BAO_TRUNCATED;
        if (blen > (zfec ? 2 * MAX_OBJECT : MAX_OBJECT)) return CHIP_ERR_INVALID_ARG;
        uint64_t olen = blen, C = 0;
        if (zfec) {
            if (blen % CHIP_FEC_M) return CHIP_ERR_UNEVEN_ZFEC_CHUNKS;  // decoding.rs:39-41
            C = blen / CHIP_FEC_M;
            if (padding[o] > CHIP_FEC_K * C) return CHIP_ERR_ZFEC;
            olen = CHIP_FEC_K * C - padding[o];  // positional shards: the primaries' bytes (decoding.rs:24-29)
        }
        const uintptr_t in = d_in + in_off[o], out = d_out + out_off[o];
        if ((in_len[o] && !d_in) || (olen && !d_out)) return CHIP_ERR_INVALID_ARG;
        if ((in % (bao ? 8 : 16)) || (out % 16)) return CHIP_ERR_INVALID_ARG;
        out_len[o] = olen;
        Obj &a = p->objs()[o];
        a.stream = reinterpret_cast<uint8_t *>(in);
        a.out = reinterpret_cast<uint8_t *>(out);
        a.C = C;
        a.n = blen;
        a.N = (uint32_t)chunks(blen);
        a.out_limit = olen;
        p->groups()[o] = (uint32_t)groups_of(format, blen);
        p->blocks()[o] = bao ? 0 : (uint32_t)((olen + COPY_BLOCK - 1) / COPY_BLOCK);
    }
    if (ranges_overlap(out_off, out_len, count)) return CHIP_ERR_INVALID_ARG;
    const int st = finish(p);
    if (st != CHIP_OK) return st;
    p->lay = ScratchLayout(count, p->total_groups);
    return CHIP_OK;
}

// bytes of device scratch a call over these lengths needs (n of encode,
// in_len of decode); lengths a call would reject count as empty
inline uint64_t scratch_len(uint8_t format, const uint64_t *len, uint64_t count, int decode) {
    uint64_t g = 0;
    for (uint64_t o = 0; len && o < count && device_format(format); ++o) {
        uint64_t n = len[o];
        if (decode) {
            if ((format & CHIP_FORMAT_BAO) && !bao_content(len[o], &n)) n = 0;
        } else if (format & CHIP_FORMAT_ZFEC) {
            n = n > MAX_OBJECT ? 0 : 8 * shard_len(n);
        }
        if (n > 2 * MAX_OBJECT) n = 0;
        g += groups_of(format, n);
    }
    return ScratchLayout(count, g).total;
}

}  // namespace ragged
}  // namespace chip
