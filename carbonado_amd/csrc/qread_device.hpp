// qread_device.hpp — one request of a device-planned ranged read into the
// tables KD's and KV's kernels are driven by (include/carbonado_hip_qread.h).
// Host/device code without a HIP type in it: qread_kernels.hip runs it one lane
// per request, and the stand-alone tests/qread_plan_check.cpp runs the same
// text on the host against read::plan_read.  The range, the segment cut, the
// slice selection and the work counts are those of read_plan.hpp
// (read::range_of, read::cut_segment) and audit_plan.hpp (audit::select):
// nothing of them is stated here a second time.
//
// Where read::plan_read packs the segments of a call, a request here owns a
// fixed number S of segment slots, [r S, (r + 1) S): the slots it does not use
// have no work items, and audit::prefix_find passes over owners without items,
// so the kernels need nothing but the prefix arrays to skip them.
#pragma once

#include "read_plan.hpp"

namespace chip {
namespace qread {

// One resident stream, as chipq_stream_table_dev uploads it.
struct StreamRec {
    uint64_t src;      // address of the stream
    uint64_t n;        // content bytes
    uint64_t N;        // chunks
    uint64_t hash;     // address of its 32-byte root
    uint32_t C;        // shard length; 0: chunk_len does not fit, or padding > 4 C
    uint32_t padding;
};
static_assert(sizeof(StreamRec) == 40, "record layout");

// What the host knows of a call: what chipq_table_info says and the capacity.
struct Shape {
    uint64_t nstreams, max_chunks, min_shard;  // chipq_table_info
    uint64_t max_len;
    uint32_t S;  // segment slots per request
};

// The tables of a call, as the kernels of KA, KD and KV read them.
struct Tables {
    read::Req *reqs;        // [nreq]
    read::Seg *segs;        // [S nreq]
    audit::Req *slices;     // [S nreq]
    uint64_t *parents;      // [S nreq + 1] counts here; qread_kernels.hip scans them in place
    uint64_t *chunks;       // [S nreq + 1]
    uint64_t *fpar;         // [S nreq + 1]
    uint64_t *blocks;       // [S nreq + 1]
    uint64_t *content_len;  // the caller's: [nreq]
};

// Request r = (stream, start, len) whose content goes to address dst.
AUDIT_HD void plan_request(const StreamRec *recs, const Shape &sh, uint32_t r, uint32_t stream, uint64_t start,
                           uint64_t len, uint64_t dst, const Tables &t) {
    read::Req q;
    q.seg0 = r * sh.S; q.nseg = 0; q.status = 0; q.pad_ = 0;
    read::Range rg;
    StreamRec rec = {0, 0, 0, 0, 0, 0};
    if (stream >= sh.nstreams || start > read::MAX_RANGE || len > read::MAX_RANGE) {
        q.status = CHIP_ERR_INVALID_ARG;
    } else {
        rec = recs[stream];
        if (rec.N > sh.max_chunks || (rec.C && rec.C < sh.min_shard)) {  // a table that is not the one info describes
            q.status = CHIP_ERR_INVALID_ARG;
        } else {
            rg = read::range_of(rec.C, rec.padding, start, len);
            q.status = rg.status;
            if (rg.end - rg.begin > sh.max_len || rg.nseg > sh.S) {  // (more segments than slots: not with C >= min_shard)
                q.status = CHIP_ERR_INVALID_ARG;
                rg = read::Range();
            }
        }
    }
    q.nseg = rg.nseg;
    t.reqs[r] = q;
    t.content_len[r] = rg.end - rg.begin;
    uint64_t x = rg.begin;
    for (uint32_t k = 0; k < sh.S; ++k) {
        const uint64_t g = (uint64_t)q.seg0 + k;
        read::Seg sg = {0, 0, 0, 0, 0, 0, 0, r};
        read::SegWork w;
        w.sel.parents = 0; w.sel.first = 0; w.sel.last = 0; w.fb_parents = 0; w.blocks = 0;
        if (k < rg.nseg) {
            w = read::cut_segment(x, rg.end, rec.C, rec.n, rec.src, dst, r, &sg);
            t.slices[g] = audit::req_of(w.sel, rec.n, rec.src, 0, rec.hash);
            dst += w.bytes;
            x += w.bytes;
        }
        t.segs[g] = sg;
        t.parents[g] = w.sel.parents;
        t.chunks[g] = w.sel.last - w.sel.first;
        t.fpar[g] = w.fb_parents;
        t.blocks[g] = w.blocks;
    }
}

}  // namespace qread
}  // namespace chip
