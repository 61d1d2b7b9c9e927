// read_plan.hpp — host side of the ranged reads (include/carbonado_hip_read.h):
// argument checks, the caller's content layout, the segments of every request,
// one slice request of KA per segment for its own primary (audit_plan.hpp; the
// 7 fallback slices of a segment are that record shifted by whole shards, which
// the gated kernels do themselves, so they cost 8 bytes of upload, not 7
// records), the 256-entry table mask -> selected shares and inverse, and the
// scratch layout.
// Pure host code without a HIP type in it, so a stand-alone program can
// exercise it under a sanitizer (tests/read_plan_check.cpp).  Host work and the
// uploaded table are O(segments): nothing is tabulated per node.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/carbonado_hip_read.h"
#include "audit_plan.hpp"
#include "repair_plan.hpp"

namespace chip {
namespace read {

constexpr uint64_t MAX_RANGE = 1ull << 53;  // start and len: start + len stays u64
constexpr uint64_t BLOCK = 4096;            // content bytes per workgroup of the read kernel
constexpr uint64_t UNIT = 16;               // content bytes per lane, on a 16-B boundary of the address
constexpr uint32_t K = repair::K, M = repair::M;
constexpr uint32_t FALLBACKS = M - 1;       // slices hashed only when a segment's own slice failed

using repair::up;

// One request, as the resolve kernel reads it (device scratch).
struct Req {
    uint32_t seg0;    // its first segment
    uint32_t nseg;    // 0 (empty, or refused below) to 4
    uint32_t status;  // decided on the host: 0, or CHIP_ERR_ZFEC for a chunk_len or padding that does not fit
    uint32_t pad_;
};
static_assert(sizeof(Req) == 16, "record layout");

// One segment: columns [c0, c1) of primary p of a stream, c0 < c1.
struct Seg {
    uint64_t src;  // address of the stream
    uint64_t dst;  // address of its first content byte
    uint32_t N;    // chunks of the stream (8 spc)
    uint32_t spc;  // chunks per shard
    uint32_t c0, c1;
    uint32_t p;
    uint32_t req;
};
static_assert(sizeof(Seg) == 40, "record layout");

// How a segment is served, written by the resolve kernel for the read kernel.
struct Served {
    uint32_t mode;  // DIRECT, REBUILT or FAILED
    uint32_t sel;   // REBUILT: byte s = the true index of selected share s
    uint32_t coef;  // REBUILT: byte s = coef[p][s]
    uint32_t pad_;
};
static_assert(sizeof(Served) == 16, "record layout");
enum : uint32_t { DIRECT = 0, REBUILT = 1, FAILED = 2 };

// mask of authentic slices -> the shares to rebuild from and their inverse
struct MaskEntry {
    uint8_t sel[4];    // the four lowest set bits
    uint8_t coef[16];  // primary p = sum_s coef[4 p + s] * share sel[s]
    uint8_t ok;        // 0: fewer than 4 bits
    uint8_t pad_[11];
};
static_assert(sizeof(MaskEntry) == 32, "record layout");

inline const std::vector<MaskEntry> &mask_table() {
    static const std::vector<MaskEntry> t = [] {
        std::vector<MaskEntry> v(256);
        for (uint32_t m = 0; m < 256; ++m) {
            MaskEntry &e = v[m];
            std::memset(&e, 0, sizeof e);
            if (__builtin_popcount(m) < (int)K) continue;
            uint32_t k = 0;
            for (uint32_t i = 0; i < M && k < K; ++i)
                if (m >> i & 1) e.sel[k++] = (uint8_t)i;
            e.ok = repair::inverse_for(e.sel, e.coef) ? 1 : 0;
        }
        return v;
    }();
    return t;
}

// ---- requests and segments -------------------------------------------------------
// What a request reads of a stream with shard length C (0: chunk_len does not
// fit) and this padding.
struct Range {
    uint32_t status = 0;         // 0 or CHIP_ERR_ZFEC
    uint64_t begin = 0, end = 0; // object bytes [begin, end); begin == end: empty
    uint32_t nseg = 0;
};
AUDIT_HD Range range_of(uint64_t C, uint32_t padding, uint64_t start, uint64_t len) {
    Range g;
    if (!C || padding > K * C) {
        g.status = CHIP_ERR_ZFEC;
        return g;
    }
    const uint64_t n_obj = K * C - padding;
    if (len == 0 || start >= n_obj) return g;
    g.begin = start;
    g.end = audit::umin(n_obj, start + len);
    g.nseg = (uint32_t)((g.end - 1) / C - g.begin / C + 1);
    return g;
}

// shard length from chunk_len alone (the layout call has no stream lengths)
inline uint64_t shard_len_alone(uint32_t chunk_len) { return chunk_len % 1024 ? 0 : chunk_len; }

inline int layout(const uint32_t *chunk_len, const uint32_t *padding, uint64_t nstreams, const uint32_t *req_stream,
                  const uint64_t *start, const uint64_t *len, uint64_t nreq, uint64_t align, uint64_t *content_off,
                  uint64_t *content_len, uint64_t *content_total, uint64_t *nseg) {
    if (align == 0 || align % 16) return CHIP_ERR_INVALID_ARG;
    if (nreq && (!chunk_len || !padding || !req_stream || !start || !len)) return CHIP_ERR_INVALID_ARG;
    uint64_t c = 0, segs = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        if (req_stream[r] >= nstreams || start[r] > MAX_RANGE || len[r] > MAX_RANGE) return CHIP_ERR_INVALID_ARG;
        const uint32_t s = req_stream[r];
        const Range g = range_of(shard_len_alone(chunk_len[s]), padding[s], start[r], len[r]);
        if (content_off) content_off[r] = c;
        if (content_len) content_len[r] = g.end - g.begin;
        c += up(g.end - g.begin, align);
        segs += g.nseg;
    }
    if (content_total) *content_total = c;
    if (nseg) *nseg = segs;
    return CHIP_OK;
}

// ---- the scratch -----------------------------------------------------------------
// [KA's table of nseg slice requests | mask table | requests | segments |
// fallback parents prefix | blocks prefix] (the uploaded table), then [8 nseg
// slice status words | how each segment is served], every region on a 256-B
// boundary.
struct ScratchLayout {
    uint64_t audit = 0, masks = 0, reqs = 0, segs = 0, fpar = 0, blocks = 0, table_end = 0, rstat = 0, served = 0,
             total = 0;
    ScratchLayout(uint64_t nreq, uint64_t nseg) {
        masks = up(audit::ScratchLayout(nseg).total, 256);
        reqs = masks + 256 * sizeof(MaskEntry);
        segs = reqs + up(nreq * sizeof(Req), 256);
        fpar = segs + up(nseg * sizeof(Seg), 256);
        blocks = fpar + up((nseg + 1) * 8, 256);
        table_end = blocks + up((nseg + 1) * 8, 256);
        rstat = table_end;
        served = rstat + up(M * nseg * 4, 256);
        total = served + up(nseg * sizeof(Served), 256);
    }
};

inline uint64_t scratch_len(uint64_t nreq, uint64_t nseg) { return ScratchLayout(nreq, nseg).total; }

// The tables of one call and the totals its launches need.
struct Plan {
    audit::Plan ka;  // ka.table, as uploaded: KA's table of the primary slices, then this header's regions
    ScratchLayout lay{0, 0};
    uint64_t nreq = 0, nseg = 0, total_blocks = 0;
    uint64_t prim_parents = 0, prim_chunks = 0;  // KA's items of the primary slices
    uint64_t fb_parents = 0;                     // fallback parent items; the fallback chunk items are 7 prim_chunks
    Req *reqs() { return reinterpret_cast<Req *>(ka.table.data() + lay.reqs); }
    Seg *segs() { return reinterpret_cast<Seg *>(ka.table.data() + lay.segs); }
    uint64_t *fpar() { return reinterpret_cast<uint64_t *>(ka.table.data() + lay.fpar); }      // [nseg + 1]
    uint64_t *blocks() { return reinterpret_cast<uint64_t *>(ka.table.data() + lay.blocks); }  // [nseg + 1]
};

// Segment g's slice of shard i over its window is its own slice request (the
// g-th of KA's table, shard p) moved by (i - p) spc chunks.  Its status word:
// word g for i == p, else one of the 7 fallback words behind all primaries',
// ascending in i.  The fallback work items of a segment: 7 x its window's
// chunks, and 7 x the most parents any of its fallback slices selects (a lane
// past its own slice's count has nothing to do).
inline uint64_t status_word(uint64_t nseg, uint64_t g, uint32_t p, uint32_t i) {
    return i == p ? g : nseg + FALLBACKS * g + (i < p ? i : i - 1);
}

// 16-B units of the addresses [a, b), b > a: partial ones at either end count
AUDIT_HD uint64_t units_of(uint64_t a, uint64_t b) { return (b - a / UNIT * UNIT + UNIT - 1) / UNIT; }

// One segment of a request and the work it brings: the request's object bytes
// from x up to the end of their primary (or of the range, `end`) of a stream of
// n = 8 C content bytes at `src`, handed out at `dst`.  The host plan below and
// the kernel that plans reads on the device (qread_device.hpp) both cut here.
struct SegWork {
    audit::Sel sel;       // the segment's own slice: its window of chunks of the stream (olen 0)
    uint64_t bytes;       // content bytes of the segment
    uint64_t fb_parents;  // fallback parent items
    uint64_t blocks;      // workgroups of the read kernel
};
AUDIT_HD SegWork cut_segment(uint64_t x, uint64_t end, uint64_t C, uint64_t n, uint64_t src, uint64_t dst, uint32_t r,
                             Seg *sg) {
    const uint64_t spc = C / 1024, pr = x / C, stop = audit::umin(end, (pr + 1) * C);
    sg->src = src; sg->dst = dst; sg->N = (uint32_t)(M * spc); sg->spc = (uint32_t)spc;
    sg->c0 = (uint32_t)(x - pr * C); sg->c1 = (uint32_t)(stop - pr * C);  // c1 <= C < 2^32
    sg->p = (uint32_t)pr; sg->req = r;
    const uint64_t w0 = sg->c0 / 1024, w1 = ((uint64_t)sg->c1 + 1023) / 1024;
    SegWork w;
    w.sel = audit::select(n, pr * spc + w0, w1 - w0);
    w.sel.olen = 0;
    uint64_t most = 0;
    for (uint64_t i = 0; i < M; ++i)
        if (i != pr) {
            const uint64_t here = audit::sel_parents(w.sel.N, i * spc + w0, i * spc + w1);
            if (here > most) most = here;
        }
    w.bytes = stop - x;
    w.fb_parents = FALLBACKS * most;
    w.blocks = (units_of(dst, dst + w.bytes) * UNIT + BLOCK - 1) / BLOCK;
    return w;
}

// Addresses are plain integers here (base + offset).  Every INVALID_ARG of a
// call is found before its first BAO_TRUNCATED is reported.
inline int plan_read(uintptr_t d_streams, const uint64_t *in_off, const uint64_t *in_len, uintptr_t d_hash,
                     const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams, const uint32_t *req_stream,
                     const uint64_t *start, const uint64_t *len, uint64_t nreq, uintptr_t d_content,
                     const uint64_t *content_off, uint64_t *content_len, bool have_results, uintptr_t d_scratch,
                     uint64_t scratch_len_given, Plan *p) {
    if (nreq == 0) return CHIP_OK;
    if (!d_streams || !in_off || !in_len || !padding || !chunk_len || !req_stream || !start || !len || !content_off ||
        !content_len || !have_results || !d_scratch)
        return CHIP_ERR_INVALID_ARG;
    if (nreq >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> n;
    bool truncated = false;
    int st = audit::stream_lengths(d_streams, in_off, in_len, nstreams, &n, &truncated);
    if (st != CHIP_OK) return st;
    // first pass: the ranges, so that the tables can be sized
    std::vector<Range> ranges(nreq);
    uint64_t nseg = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        if (req_stream[r] >= nstreams || start[r] > MAX_RANGE || len[r] > MAX_RANGE) return CHIP_ERR_INVALID_ARG;
        const uint32_t s = req_stream[r];
        ranges[r] = range_of(repair::shard_len_of(n[s], chunk_len[s]), padding[s], start[r], len[r]);
        if ((d_content + content_off[r]) % 16) return CHIP_ERR_INVALID_ARG;
        content_len[r] = ranges[r].end - ranges[r].begin;
        if (content_len[r] && !d_content) return CHIP_ERR_INVALID_ARG;
        nseg += ranges[r].nseg;
    }
    if (d_scratch % 16) return CHIP_ERR_INVALID_ARG;
    if (audit::ranges_overlap(content_off, content_len, nreq)) return CHIP_ERR_INVALID_ARG;
    if (nseg >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;  // slice requests: one kind of work item

    p->nreq = nreq;
    p->nseg = nseg;
    p->lay = ScratchLayout(nreq, nseg);
    audit::start(&p->ka, nseg);
    p->ka.table.resize(p->lay.table_end, 0);
    std::memcpy(p->ka.table.data() + p->lay.masks, mask_table().data(), 256 * sizeof(MaskEntry));
    uint64_t g = 0, b = 0, fp = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        const Range &rg = ranges[r];
        const uint32_t s = req_stream[r];
        Req &q = p->reqs()[r];
        q.seg0 = (uint32_t)g; q.nseg = rg.nseg; q.status = rg.status; q.pad_ = 0;
        if (!rg.nseg) continue;
        const uint64_t C = chunk_len[s], src = d_streams + in_off[s];
        uint64_t dst = d_content + content_off[r];
        for (uint64_t x = rg.begin; x < rg.end; ++g) {
            const SegWork w = cut_segment(x, rg.end, C, n[s], src, dst, (uint32_t)r, &p->segs()[g]);
            audit::put(&p->ka, g, w.sel, n[s], src, 0, d_hash + 32 * s, 0);
            p->fpar()[g] = fp;
            fp += w.fb_parents;
            p->blocks()[g] = b;
            b += w.blocks;
            dst += w.bytes;
            x += w.bytes;
        }
    }
    p->fpar()[nseg] = fp;
    p->fb_parents = fp;
    p->blocks()[nseg] = b;
    p->total_blocks = b;
    st = audit::finish(&p->ka);
    if (st != CHIP_OK) return st;
    if (fp >= audit::MAX_ITEMS || FALLBACKS * p->ka.total_chunks >= audit::MAX_ITEMS || b >= (1ull << 31))
        return CHIP_ERR_INVALID_ARG;
    if (scratch_len_given < p->lay.total) return CHIP_ERR_INVALID_ARG;
    p->prim_parents = p->ka.total_parents;
    p->prim_chunks = p->ka.total_chunks;
    if (truncated) return CHIP_ERR_BAO_TRUNCATED;
    return d_hash ? CHIP_OK : CHIP_ERR_HASH_DECODE;
}

}  // namespace read
}  // namespace chip
