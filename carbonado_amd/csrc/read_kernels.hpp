// read_kernels.hpp — launch interface of read_kernels.hip (KD) for
// api_read.cpp and api_vread.cpp.  The tables it points to are laid out by read_plan.hpp.
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
    bool bounded;                // the device-planned reads: nseg counts slots, the totals are bounds (qread_plan.hpp)
};

// The launch table of a plan whose uploaded table lies at the start of the
// scratch `scr`; `status` and `used` are the caller's.
inline ReadLaunch read_launch_of(const read::Plan &p, uint8_t *scr, uint32_t *status, uint32_t *used) {
    const audit::ScratchLayout &ka = p.ka.lay;
    ReadLaunch L{};
    L.slices = reinterpret_cast<const audit::Req *>(scr + p.lay.audit + ka.reqs);
    L.parents = reinterpret_cast<const uint64_t *>(scr + p.lay.audit + ka.parents);
    L.chunks = reinterpret_cast<const uint64_t *>(scr + p.lay.audit + ka.chunks);
    L.masks = reinterpret_cast<const read::MaskEntry *>(scr + p.lay.masks);
    L.reqs = reinterpret_cast<const read::Req *>(scr + p.lay.reqs);
    L.segs = reinterpret_cast<const read::Seg *>(scr + p.lay.segs);
    L.fpar = reinterpret_cast<const uint64_t *>(scr + p.lay.fpar);
    L.blocks = reinterpret_cast<const uint64_t *>(scr + p.lay.blocks);
    L.rstat = reinterpret_cast<uint32_t *>(scr + p.lay.rstat);
    L.served = reinterpret_cast<read::Served *>(scr + p.lay.served);
    L.nreq = p.nreq; L.nseg = p.nseg; L.total_blocks = p.total_blocks;
    L.prim_parents = p.prim_parents; L.prim_chunks = p.prim_chunks; L.fb_parents = p.fb_parents;
    L.status = status; L.used = used;
    return L;
}

// Enqueue the fallback slices' checks, each gated on its segment's own slice
// (two launches, behind KA's checks of the primary slices).  pathw = NULL: the
// gate reads the segment's primary status word (the ranged reads); else it also
// reads its path word of pathw[nseg] (the vouched reads).
hipError_t read_fallback_launch(const ReadLaunch &L, const uint32_t *pathw, hipStream_t stream);

// Enqueue the verdict per request and segment, then the read itself (two launches).
hipError_t read_serve_launch(const ReadLaunch &L, hipStream_t stream);

// Enqueue the read alone, for a caller that has written `served` and the
// status words itself (the vouched reads; one launch).
hipError_t read_copy_launch(const ReadLaunch &L, hipStream_t stream);

}  // namespace chip
