// vread_plan.hpp — host side of the vouched ranged reads
// (include/carbonado_hip_vread.h).  A vouched read is a ranged read
// (read_plan.hpp: the same checks in the same order, the same segments, slice
// requests, mask table and uploaded table) with two more words per segment
// behind its scratch and one more kind of work item: a VOUCH ITEM per
// (segment, window chunk).  The vouch items are numbered by the chunk prefix of
// the primary slices that the plan already uploads (audit::Plan::chunks()):
// items [pre[g], pre[g + 1]) are segment g's, item i is chunk
// w0 + (i - pre[g]) of its primary; no new prefix array is built.
// Pure host code without a HIP type in it (tests/vread_plan_check.cpp drives it
// under a sanitizer).
#pragma once

#include "../../include/carbonado_hip_vread.h"
#include "read_plan.hpp"

namespace chip {
namespace vread {

using read::up;

// [the scratch of a ranged read | path word per segment | contradiction word
// per segment].  The words from read's rstat to the end are zeroed by one
// memset (read's `served` records lie among them and are written later).
struct ScratchLayout {
    read::ScratchLayout rd{0, 0};
    uint64_t path = 0, contra = 0, total = 0;
    ScratchLayout(uint64_t nreq, uint64_t nseg) : rd(nreq, nseg) {
        path = rd.total;
        contra = path + up(nseg * 4, 256);
        total = contra + up(nseg * 4, 256);
    }
    uint64_t zero_from() const { return rd.rstat; }
    uint64_t zero_len() const { return total - rd.rstat; }
};

inline uint64_t scratch_len(uint64_t nreq, uint64_t nseg) { return ScratchLayout(nreq, nseg).total; }

struct Plan {
    read::Plan rd;
    ScratchLayout lay{0, 0};
    uint64_t vouch_items = 0;  // = rd.prim_chunks
};

// The checks of read::plan_read in its order, with d_vouch among the NULL
// checks, the flags behind them, and this header's scratch length in the place
// of read's.
inline int plan_vread(uintptr_t d_streams, const uint64_t *in_off, const uint64_t *in_len, uintptr_t d_hash,
                      const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams, const uint32_t *req_stream,
                      const uint64_t *start, const uint64_t *len, uint64_t nreq, uintptr_t d_content,
                      const uint64_t *content_off, uint64_t *content_len, bool have_results, uint32_t flags,
                      uintptr_t d_scratch, uint64_t scratch_len_given, Plan *p) {
    if (nreq == 0) return CHIP_OK;
    if (!d_streams || !in_off || !in_len || !padding || !chunk_len || !req_stream || !start || !len || !content_off ||
        !content_len || !have_results || !d_scratch)
        return CHIP_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)CHIPV_STRICT) return CHIP_ERR_INVALID_ARG;
    // read's own scratch check is its last INVALID_ARG: it cannot fail here, ours takes its place
    const int st = read::plan_read(d_streams, in_off, in_len, d_hash, padding, chunk_len, nstreams, req_stream, start,
                                   len, nreq, d_content, content_off, content_len, have_results, d_scratch, ~0ull,
                                   &p->rd);
    if (st == CHIP_ERR_INVALID_ARG) return st;
    p->lay = ScratchLayout(nreq, p->rd.nseg);
    p->vouch_items = p->rd.prim_chunks;
    if (scratch_len_given < p->lay.total) return CHIP_ERR_INVALID_ARG;
    return st;
}

}  // namespace vread
}  // namespace chip
