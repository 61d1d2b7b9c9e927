// qread_kernels.hpp — launch interface of qread_kernels.hip (KQ) for
// api_qread.cpp.  The tables it points to are laid out by qread_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "qread_plan.hpp"

namespace chip {

struct QreadLaunch {
    const qread::StreamRec *recs;  // device: the stream table's records
    qread::Shape shape;
    const uint32_t *req_stream;    // device, the caller's: [nreq]
    const uint64_t *start, *len;   // device, the caller's: [nreq] each
    uint64_t nreq;
    uint64_t content, stride;      // request r's content goes to address content + r stride
    qread::Tables tables;          // device; the four prefix arrays lie `pitch` entries apart, parents first
    uint64_t pitch;
    uint32_t *rstat;               // device: [8 S nreq] status word per slice, zeroed by the plan
    uint32_t *pathw, *contra;      // device: [S nreq] each, zeroed by the plan; NULL: the unvouched call
    uint64_t *sums;                // device: [4][scan_blocks] workgroup sums of the scan
    uint64_t scan_blocks;
};

// Enqueue the plan of a call: one lane per request, then the exclusive scan of
// the four count arrays in place (four launches; no workgroup waits on another).
hipError_t qread_plan_launch(const QreadLaunch &L, hipStream_t stream);

}  // namespace chip
