// read_kernels.hpp — launch interface of read_kernels.hip (KD) for
// api_read.cpp.  The tables it points to are laid out by read_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "read_plan.hpp"

namespace chip {

struct ReadLaunch {
    const audit::Req *slices;    // device: [nseg] each segment's own slice request
    const uint64_t *parents;     // device: [nseg + 1] prefix of selected parents per slice request
    const uint64_t *chunks;      // device: [nseg + 1] prefix of selected chunks per slice request
    const uint64_t *fpar;        // device: [nseg + 1] prefix of fallback parent items per segment
    const read::MaskEntry *masks;  // device: [256]
    const read::Req *reqs;       // device: [nreq]
    const read::Seg *segs;       // device: [nseg]
    const uint64_t *blocks;      // device: [nseg + 1] prefix of read-kernel workgroups per segment
    uint32_t *rstat;             // device: [8 nseg] status word per slice (read::status_word), zero at launch
    read::Served *served;        // device: [nseg]
    uint64_t nreq, nseg, total_blocks;
    uint64_t prim_parents, prim_chunks, fb_parents;
    uint32_t *status, *used;     // the caller's: [nreq] each
};

// Enqueue the fallback slices' checks, each gated on its segment's primary
// status word (two launches, behind KA's checks of the primary slices).
hipError_t read_fallback_launch(const ReadLaunch &L, hipStream_t stream);

// Enqueue the verdict per request and segment, then the read itself (two launches).
hipError_t read_serve_launch(const ReadLaunch &L, hipStream_t stream);

// Enqueue the read alone, for a caller that has written `served` and the
// status words itself (the vouched reads; one launch).
hipError_t read_copy_launch(const ReadLaunch &L, hipStream_t stream);

}  // namespace chip
