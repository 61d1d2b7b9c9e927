// gread_kernels.hpp — launch interface of gread_kernels.hip (KG) for
// api_gread.cpp.  The tables it points to are laid out by gread_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "gread_plan.hpp"

namespace chip {

struct GreadLaunch {
    const qread::StreamRec *recs;    // device: the stream table's records
    const gread::FrameRec *frecs;    // device: the frame table's records, [nstreams]
    const uint64_t *ent;             // device: the frame table's entries
    const uint32_t *key_status;      // device: the key table's words, [nstreams]; NULL at 14
    gread::Shape shape;
    const uint32_t *req_stream;      // device, the caller's: [nreq]
    const uint64_t *start, *len;     // device, the caller's: [nreq] each, plaintext bytes
    uint32_t *q_stream;              // device, the call's scratch: the frame-stream requests, [nreq] each
    uint64_t *q_start, *q_len;
    uint32_t *bad;                   // device, the call's scratch: [nreq fcap]
    const uint8_t *stage;            // device, the call's scratch: slot r at stage + r stage_stride
    uint64_t stage_stride;
    uint32_t nreq;
    uint8_t *content;                // request r's content is at content + r stride
    uint64_t stride;
    uint64_t *content_len;           // the caller's: written by the finish kernel
    uint32_t *status, *used, *vouch; // the inner read's result words: the gate; rewritten by the finish kernel
};

// One lane per request: the frame-stream request into the call's scratch.
hipError_t gread_rewrite_launch(const GreadLaunch &L, hipStream_t stream);
// One workgroup per (request, k): frame f0 + k, gated on the request's status
// word: header against the index, block decode in LDS, CRC, the wanted bytes stored.
hipError_t gread_block_launch(const GreadLaunch &L, hipStream_t stream);
// One workgroup per request: the frames' verdicts combined; a failed or killed
// request zeroed; the content length of every request.
hipError_t gread_finish_launch(const GreadLaunch &L, hipStream_t stream);

}  // namespace chip
