// gread_device.hpp — one plaintext request of a device-planned level-14 /
// level-15 read (include/carbonado_hip_gread.h): what becomes of it, the
// frame-stream request the inner planned read gets in its place, and the
// (request, frame) work item of the block decode, built from the request and the
// resident frame table.  Host/device code without a HIP type in it:
// gread_kernels.hip runs decide() one lane per request (the rewrite), once per
// workgroup of the block decode and once per workgroup of the finish, and the
// stand-alone tests/gread_plan_check.cpp runs the same text on the host against
// fread::plan_ranges and fread::plan_items.  The range of the frame-stream
// request in the object is read::range_of, the record checks are those of
// qread::plan_request, and at 15 the inner call's own decision is
// kread::decide: nothing of them is stated here a second time.
//
// Everything this text looks at is public: stream indices, positions, lengths,
// the stream records, the frame records and entries, the key_status words.  It
// touches no key.
#pragma once

#include "fread_device.hpp"
#include "kread_device.hpp"

namespace chip {
namespace gread {

using fread::FRAME;

constexpr uint32_t NO_STREAM = kread::NO_STREAM;  // a stream index the inner planner refuses

constexpr uint32_t REFUSED = 1;  // order 1 of the header: CHIP_ERR_INVALID_ARG, nothing read
constexpr uint32_t KILLED = 2;   // order 2: the stream's index_status, zeros over the clipped range
constexpr uint32_t READ = 3;     // orders 3 and 4: the inner planned read of the frames, then the block decode

// One stream of the frame table, as chipg_frame_table_dev uploads it.
struct FrameRec {
    uint64_t ent0;          // its first entry among the table's entries (index_status 0 only)
    uint64_t nframes;       // it has nframes + 1 entries
    uint64_t plain_len;
    uint32_t index_status;  // not 0: killed, no entries
    uint32_t pad_;
};
static_assert(sizeof(FrameRec) == 32, "record layout");

// What the host knows of a call: chipg_frame_info, the capacity and the inner call's shape.
struct Shape {
    uint64_t nstreams, nentries, max_frame;  // chipg_frame_info
    uint64_t max_len;                        // the outer capacity, plaintext bytes
    uint32_t fcap;                           // frames a request may touch
    uint32_t keyed;                          // format 15: the inner call is kread's
    qread::Shape inner;                      // of the inner planned read: max_len' = fcap max_frame
};

// frames a range of max_len >= 1 bytes can touch: it starts at most 65535 bytes into its first
AUDIT_HD uint64_t fcap_of(uint64_t max_len) { return (max_len + (FRAME - 2)) / FRAME + 1; }

struct Decision {
    uint32_t order;
    uint32_t kill;      // KILLED: the index_status word
    uint64_t b, n;      // the clipped plaintext range [b, b + n); n == 0: empty
    uint64_t f0;        // READ and n != 0: its first frame, and how many it touches
    uint32_t nfr;
    uint32_t q_stream;  // the frame-stream request the inner planner gets
    uint64_t q_start, q_len;
};

// The inner planned call's refusals of request (stream, start, len) over its own capacity.
AUDIT_HD bool inner_refuses(const qread::StreamRec *recs, const uint32_t *key_status, const Shape &sh, uint32_t stream,
                            uint64_t start, uint64_t len) {
    if (sh.keyed) return kread::decide(recs, key_status, sh.inner, stream, start, len).order == kread::REFUSED;
    const qread::StreamRec rec = recs[stream];  // as qread::plan_request
    if (rec.N > sh.inner.max_chunks || (rec.C && rec.C < sh.inner.min_shard)) return true;
    const read::Range rg = read::range_of(rec.C, rec.padding, start, len);
    return rg.end - rg.begin > sh.inner.max_len || rg.nseg > sh.inner.S;
}

// Request (stream, start, len) in plaintext bytes.  ent: the table's entries.
AUDIT_HD Decision decide(const qread::StreamRec *recs, const FrameRec *frecs, const uint64_t *ent,
                         const uint32_t *key_status, const Shape &sh, uint32_t stream, uint64_t start, uint64_t len) {
    Decision d = {REFUSED, 0, 0, 0, 0, 0, NO_STREAM, 0, 0};
    if (stream >= sh.nstreams || start > read::MAX_RANGE || len > read::MAX_RANGE) return d;
    const FrameRec fr = frecs[stream];
    const uint64_t P = fr.plain_len;
    const uint64_t n = (!len || start >= P) ? 0 : (P - start < len ? P - start : len);  // as fread::plan_ranges
    if (n > sh.max_len) return d;
    uint64_t q_start = 0, q_len = 0, f0 = 0;
    uint32_t nfr = 0;
    if (!fr.index_status) {
        if (fr.ent0 > sh.nentries || fr.nframes >= sh.nentries - fr.ent0) return d;  // entries past the table's
        if (n) {
            const uint64_t *off = ent + fr.ent0;
            const uint64_t f1 = (start + n - 1) / FRAME;
            f0 = start / FRAME;
            // plain_len does not fit nframes: not a table chipg_frame_table_dev made
            if (f1 >= fr.nframes || P > uint64_t(FRAME) * fr.nframes) return d;
            for (uint64_t f = f0; f <= f1; ++f)  // fcap frames or fewer: n <= max_len
                if (off[f + 1] < off[f] || off[f + 1] - off[f] > sh.max_frame) return d;
            nfr = uint32_t(f1 - f0 + 1);
            q_start = off[f0];
            q_len = off[f1 + 1] - off[f0];
        }
    }
    if (inner_refuses(recs, key_status, sh, stream, q_start, q_len)) return d;
    d.b = start;
    d.n = n;
    d.q_stream = stream;
    if (fr.index_status) {  // no hashing, no keystream, no decode: the planner sees an empty request
        d.order = KILLED;
        d.kill = fr.index_status;
        return d;
    }
    d.order = READ;
    d.f0 = f0;
    d.nfr = nfr;
    d.q_start = q_start;
    d.q_len = q_len;
    return d;
}

// ---- the bounded work mapping ------------------------------------------------------
// Workgroup w of the block decode is (request, k) = (w % nreq, w / nreq) and has
// frame f0 + k of its request; one with k >= nfr leaves at once.  Its fread::Seg,
// built where the kernel builds it: no table.  stage_stride: of the inner read's
// slots, whose slot r holds frame-stream bytes [off[f0], off[f1 + 1]).
AUDIT_HD fread::Seg item_of_request(const FrameRec &fr, const uint64_t *ent, const Decision &d, uint64_t r, uint32_t k,
                                    uint64_t stage_stride, uint64_t content_stride) {
    const uint64_t *off = ent + fr.ent0;
    const uint64_t f = d.f0 + k, b = d.b, e = d.b + d.n;
    const uint64_t lo = b > uint64_t(FRAME) * f ? b - uint64_t(FRAME) * f : 0;
    const uint64_t hi = e < uint64_t(FRAME) * (f + 1) ? e - uint64_t(FRAME) * f : FRAME;
    const uint64_t room = off[f + 1] - off[f];
    fread::Seg sg;
    sg.src = r * stage_stride + (off[f] - off[d.f0]);
    sg.dst = r * content_stride + (uint64_t(FRAME) * f + lo - b);
    sg.req = uint32_t(r);
    sg.clen = room >= 8 && room - 4 < (uint64_t(1) << 24) ? uint32_t(room - 4) : 0;
    sg.ulen = uint32_t(f + 1 == fr.nframes ? fr.plain_len - uint64_t(FRAME) * f : FRAME);
    sg.lo = uint32_t(lo);
    sg.hi = uint32_t(hi);
    sg.pad_ = 0;
    return sg;
}

}  // namespace gread
}  // namespace chip
