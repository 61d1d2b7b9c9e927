// fread_plan.hpp — host logic of include/carbonado_hip_fread.h: the length of
// a stream's frame stream, the scratch layouts, the header reads an index
// check makes, and the read's requests, staging rows and (request, frame) work
// items.  Pure host code (no HIP): it is compiled into api_fread.cpp and,
// stand-alone under ASan + UBSan, into tests/fread_plan_check.cpp.
//
// Scratch of the index calls, in this order (every region 16-B aligned):
//   walk streams | raw keys | CtrKeys      (the walk's table and key region)
//   walk results | walked offsets          (one copy back)
//   chain streams | offsets                (one upload)
//   rows, 16 B per entry | status, used and vouch word per entry
//   status, vouch (4 B) and plain_len (8 B) per stream   (one copy back)
//   the vouched read's scratch | the keystream call's scratch
// Scratch of a read:
//   staging rows | requests | work items | a verdict word per work item
//   the vouched read's scratch | the keystream call's scratch
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/carbonado_hip_fread.h"
#include "cread_plan.hpp"
#include "fread_device.hpp"
#include "stream_rules.hpp"
#include "vread_plan.hpp"

namespace chip {
namespace fread {

using rules::up16;

constexpr uint64_t ENV = cread::ENV_OVERHEAD;
constexpr uint64_t MAX_STREAMS = uint64_t(1) << 31;
constexpr uint64_t MAX_ENTRIES = uint64_t(1) << 30;
constexpr uint64_t MAX_RANGE = read::MAX_RANGE;

inline bool format_ok(uint8_t format) { return format == 14 || format == 15; }
inline uint64_t shift_of(uint8_t format) { return format == 15 ? ENV : 0; }

// bytes of the frame stream of a stream with this chunk_len and padding (0
// where they do not fit, as the ranged reads see them)
inline uint64_t stream_len(uint32_t chunk_len, uint32_t padding, uint64_t shift) {
    const uint64_t C = read::shard_len_alone(chunk_len);
    if (!C || padding > read::K * C) return 0;
    const uint64_t obj = read::K * C - padding;
    return obj > shift ? obj - shift : 0;
}

// ---- the index calls --------------------------------------------------------------
struct IndexLayout {
    uint64_t wstreams = 0, rawkeys = 0, km = 0, wout = 0, woff = 0, vtab = 0, voff = 0, rows = 0, rstat = 0, rused = 0,
             rvouch = 0, ostat = 0, ovouch = 0, oplain = 0, vread = 0, ctr = 0, total = 0;
    uint64_t out_len = 0;  // of [ostat, oplain end)
    IndexLayout(uint64_t ns, uint64_t ne) {
        rawkeys = up16(ns * sizeof(WStream));
        km = rawkeys + ns * cread::RAW_KEY;
        wout = km + ns * sizeof(cread::CtrKey);
        woff = wout + up16(ns * sizeof(WalkOut));
        vtab = woff + up16(ne * 8);
        voff = vtab + up16(ns * sizeof(VStream));
        rows = voff + up16(ne * 8);
        rstat = rows + ne * ROW;
        rused = rstat + up16(ne * 4);
        rvouch = rused + up16(ne * 4);
        ostat = rvouch + up16(ne * 4);
        ovouch = ostat + up16(ns * 4);
        oplain = ovouch + up16(ns * 4);
        out_len = oplain + ns * 8 - ostat;
        vread = up16(oplain + ns * 8);
        ctr = vread + up16(vread::scratch_len(ne, 2 * ne));
        total = ctr + cread::scratch_len(ns, ne);
    }
    uint64_t wipe_from() const { return rawkeys; }
    uint64_t wipe_len() const { return wout - rawkeys; }
};

inline uint64_t index_scratch_len(uint64_t ns, uint64_t ne) {
    if (ns >= MAX_STREAMS || ne >= MAX_ENTRIES) return 0;
    return IndexLayout(ns, ne).total;
}

// What a stream is to the index calls, from host arrays alone.
struct Geo {
    uint64_t L = 0;       // bytes of its frame stream
    uint32_t N = 0;       // chunks of its bao stream
    uint32_t status = 0;  // CHIP_ERR_ZFEC where chunk_len or padding does not fit the stream
};
inline Geo geo_of(uint64_t content, uint32_t chunk_len, uint32_t padding, uint64_t shift) {
    Geo g;
    if (content == 0 && chunk_len == 0 && padding == 0 && shift == 0) {  // the empty object at 14: an empty frame stream
        g.N = 1;
        return g;
    }
    const uint64_t C = repair::shard_len_of(content, chunk_len);
    if (!C || padding > read::K * C) {
        g.status = CHIP_ERR_ZFEC;
        return g;
    }
    g.N = uint32_t(read::M * C / 1024);
    g.L = stream_len(chunk_len, padding, shift);
    return g;
}

// The header reads of an index check: for every stream the identifier, then one
// read per frame, compact in stream order; request i's row is row i.
struct VerifyPlan {
    uint64_t nreq = 0;
    std::vector<uint32_t> req_stream;
    std::vector<uint64_t> start, len, coff, clen, pos;  // start: object bytes; pos: frame-stream bytes (the keystream's)
    std::vector<uint8_t> table;                          // VStream[ns] | offsets[nreq], as uploaded
    uint64_t offsets_at = 0;
};

// offs: the entries of every stream, nfr[s] + 1 each, in stream order.  skip[s]
// != 0: that status, no read.
inline void plan_verify(const std::vector<uint64_t> &offs, const std::vector<uint32_t> &nfr,
                        const std::vector<uint32_t> &skip, const std::vector<Geo> &geo, uint64_t shift,
                        VerifyPlan *p) {
    const uint64_t ns = nfr.size(), ne = offs.size();
    p->nreq = ne;
    p->req_stream.resize(ne);
    p->start.assign(ne, 0);
    p->len.assign(ne, 0);
    p->coff.resize(ne);
    p->clen.assign(ne, 0);
    p->pos.assign(ne, 0);
    p->offsets_at = up16(ns * sizeof(VStream));
    p->table.assign(p->offsets_at + ne * 8, 0);
    uint64_t e = 0;
    for (uint64_t s = 0; s < ns; ++s) {
        VStream v{};
        v.L = geo[s].L;
        v.ent0 = e;
        v.nframes = nfr[s];
        v.skip = skip[s];
        std::memcpy(p->table.data() + s * sizeof(VStream), &v, sizeof v);
        for (uint64_t f = 0; f <= nfr[s]; ++f, ++e) {
            p->req_stream[e] = uint32_t(s);
            p->coff[e] = e * ROW;
            std::memcpy(p->table.data() + p->offsets_at + e * 8, &offs[e], 8);
            if (v.skip) continue;
            // request 0 reads the identifier, request 1 + f the header at entry f
            const uint64_t at = f == 0 ? 0 : offs[e - 1], want = f == 0 ? ID_LEN : HDR_READ;
            if (at >= v.L) continue;  // nothing to read: the chain check sees the entry
            p->pos[e] = at;
            p->start[e] = shift + at;
            p->len[e] = v.L - at < want ? v.L - at : want;
        }
    }
}

// ---- the read -------------------------------------------------------------------------
struct ReadLayout {
    uint64_t rows = 0, reqs = 0, segs = 0, bad = 0, vread = 0, ctr = 0, total = 0;
    ReadLayout(uint64_t nreq, uint64_t nseg, uint64_t stage_total, uint64_t vseg, uint64_t ns) {
        reqs = up16(stage_total);
        segs = reqs + nreq * sizeof(Req);
        bad = segs + up16(nseg * sizeof(Seg));
        vread = bad + up16(nseg * 4);
        ctr = vread + up16(vread::scratch_len(nreq, vseg));
        total = ctr + cread::scratch_len(ns, nreq);
    }
};

inline uint64_t read_scratch_len(uint64_t nreq, uint64_t nseg, uint64_t stage_total, uint64_t vseg, uint64_t ns) {
    if (nreq >= cread::MAX_ITEMS || nseg >= (uint64_t(1) << 31) || stage_total > MAX_RANGE) return 0;
    return ReadLayout(nreq, nseg, stage_total, vseg, ns).total;
}

// an index the read can use: entries ascend, the last one is L, and plain_len
// fits the number of frames
inline bool index_fits(const uint64_t *off, uint64_t nframes, uint64_t plain_len, uint64_t L) {
    if (nframes >= (uint64_t(1) << 31)) return false;
    for (uint64_t f = 0; f < nframes; ++f)
        if (off[f] >= off[f + 1]) return false;
    if (off[nframes] != L) return false;
    if (nframes == 0) return plain_len == 0;
    return plain_len > FRAME * (nframes - 1) && plain_len <= FRAME * nframes;
}

struct ReadPlan {
    uint64_t nreq = 0, nseg = 0, stage_total = 0, vseg = 0;
    std::vector<uint64_t> begin, end;               // plaintext [begin, end) of every request; equal: empty
    std::vector<uint64_t> vstart, vlen, vcoff, pos;  // the vouched read's requests: object bytes into staging rows
    std::vector<uint8_t> table;                      // Req[nreq] | Seg[nseg], as uploaded (built by plan_items)
};

// The ranges, the staging rows and the totals; no table.  kill: per stream, may
// be NULL.  The arrays have been checked (req_stream[r] < nstreams, start and
// len <= 2^53, index_fits for every stream that is not killed).
inline void plan_ranges(const uint32_t *chunk_len, const uint32_t *padding, const uint64_t *frame_off,
                        const uint64_t *idx_off, const uint64_t *plain_len, const uint32_t *kill, uint64_t shift,
                        const uint32_t *req_stream, const uint64_t *start, const uint64_t *len, uint64_t nreq,
                        ReadPlan *p) {
    p->nreq = nreq;
    p->begin.assign(nreq, 0);
    p->end.assign(nreq, 0);
    p->vstart.assign(nreq, 0);
    p->vlen.assign(nreq, 0);
    p->vcoff.assign(nreq, 0);
    p->pos.assign(nreq, 0);
    uint64_t stage = 0, nseg = 0, vseg = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        const uint32_t s = req_stream[r];
        p->vcoff[r] = stage;
        const uint64_t P = plain_len[s];
        if (!len[r] || start[r] >= P) continue;
        const uint64_t b = start[r], e = P - b < len[r] ? P : b + len[r];
        p->begin[r] = b;
        p->end[r] = e;
        if (kill && kill[s]) continue;  // it claims its range and reads nothing
        const uint64_t *off = frame_off + idx_off[s];
        const uint64_t f0 = b / FRAME, f1 = (e - 1) / FRAME;
        p->pos[r] = off[f0];
        p->vstart[r] = shift + off[f0];
        p->vlen[r] = off[f1 + 1] - off[f0];
        stage += up16(p->vlen[r]);
        nseg += f1 - f0 + 1;
        vseg += read::range_of(read::shard_len_alone(chunk_len[s]), padding[s], p->vstart[r], p->vlen[r]).nseg;
    }
    p->stage_total = stage;
    p->nseg = nseg;
    p->vseg = vseg;
}

// The uploaded table of a planned read.  content_off: the caller's.
inline void plan_items(const uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *nframes,
                       const uint64_t *plain_len, const uint32_t *kill, const uint32_t *req_stream,
                       const uint64_t *content_off, ReadPlan *p) {
    const uint64_t nreq = p->nreq;
    p->table.assign(nreq * sizeof(Req) + p->nseg * sizeof(Seg), 0);
    uint64_t g = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        const uint32_t s = req_stream[r];
        Req q{};
        q.dst = content_off[r];
        q.n = p->end[r] - p->begin[r];
        q.seg0 = uint32_t(g);
        q.kill = kill ? kill[s] : 0;
        if (!q.kill && p->end[r] > p->begin[r]) {
            const uint64_t *off = frame_off + idx_off[s];
            const uint64_t b = p->begin[r], e = p->end[r], f0 = b / FRAME, f1 = (e - 1) / FRAME;
            for (uint64_t f = f0; f <= f1; ++f, ++g) {
                Seg sg{};
                const uint64_t lo = b > FRAME * f ? b - FRAME * f : 0;
                const uint64_t hi = e < FRAME * (f + 1) ? e - FRAME * f : FRAME;
                const uint64_t room = off[f + 1] - off[f];
                sg.src = p->vcoff[r] + (off[f] - off[f0]);
                sg.dst = content_off[r] + (FRAME * f + lo - b);
                sg.req = uint32_t(r);
                sg.clen = room >= 8 && room - 4 < (uint64_t(1) << 24) ? uint32_t(room - 4) : 0;
                sg.ulen = uint32_t(f + 1 == nframes[s] ? plain_len[s] - FRAME * f : FRAME);
                sg.lo = uint32_t(lo);
                sg.hi = uint32_t(hi);
                std::memcpy(p->table.data() + nreq * sizeof(Req) + g * sizeof(Seg), &sg, sizeof sg);
            }
            q.nseg = uint32_t(g) - q.seg0;
        }
        std::memcpy(p->table.data() + r * sizeof(Req), &q, sizeof q);
    }
}

// The host checks of the read's own arrays, in the header's order, behind its
// NULL checks: the format, the flags, the counts, the requests, the indexes.
inline int check_reads(uint8_t format, uint32_t flags, const uint32_t *chunk_len, const uint32_t *padding,
                       const uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *nframes,
                       const uint64_t *plain_len, const uint32_t *kill, uint64_t nstreams, const uint32_t *req_stream,
                       const uint64_t *start, const uint64_t *len, uint64_t nreq) {
    if (!format_ok(format)) return CHIP_ERR_INVALID_ARG;
    if (flags & ~uint32_t(CHIPV_STRICT)) return CHIP_ERR_INVALID_ARG;
    if (nreq >= cread::MAX_ITEMS || nstreams >= MAX_STREAMS) return CHIP_ERR_INVALID_ARG;
    for (uint64_t r = 0; r < nreq; ++r)
        if (req_stream[r] >= nstreams || start[r] > MAX_RANGE || len[r] > MAX_RANGE) return CHIP_ERR_INVALID_ARG;
    const uint64_t shift = shift_of(format);
    for (uint64_t s = 0; s < nstreams; ++s) {
        if (kill && kill[s]) continue;
        if (idx_off[s] > MAX_RANGE || nframes[s] >= (uint64_t(1) << 31)) return CHIP_ERR_INVALID_ARG;
        if (!index_fits(frame_off + idx_off[s], nframes[s], plain_len[s], stream_len(chunk_len[s], padding[s], shift)))
            return CHIP_ERR_INVALID_ARG;
    }
    return CHIP_OK;
}

// content offsets and lengths of the requests, `align` between them
inline void layout_content(const ReadPlan &p, uint64_t align, uint64_t *content_off, uint64_t *content_len,
                           uint64_t *content_total) {
    uint64_t c = 0;
    for (uint64_t r = 0; r < p.nreq; ++r) {
        if (content_off) content_off[r] = c;
        if (content_len) content_len[r] = p.end[r] - p.begin[r];
        c += rules::up(p.end[r] - p.begin[r], align);
    }
    if (content_total) *content_total = c;
}

}  // namespace fread
}  // namespace chip
