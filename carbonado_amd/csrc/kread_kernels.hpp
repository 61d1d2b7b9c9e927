// kread_kernels.hpp — launch interface of kread_kernels.hip (KK) for
// api_kread.cpp.  The tables it points to are laid out by kread_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "kread_plan.hpp"

namespace chip {

struct KreadLaunch {
    const qread::StreamRec *recs;    // device: the stream table's records
    qread::Shape shape;
    const cread::CtrKey *km;         // device: the key table's records, [nstreams]
    const uint32_t *key_status;      // device: the key table's words, [nstreams]
    const uint32_t *req_stream;      // device, the caller's: [nreq]
    const uint64_t *start, *len;     // device, the caller's: [nreq] each, plaintext bytes
    uint32_t *q_stream;              // device, the call's scratch: the envelope requests, [nreq] each
    uint64_t *q_start, *q_len;
    uint32_t nreq, cap;              // cap: spans per request
    uint8_t *content;                // request r's content is at content + r stride
    uint64_t stride;
    uint64_t *content_len;           // the caller's: written by the plan; by the keystream kernel for a killed request
    uint32_t *status, *used, *vouch; // the read's result words: the gate; written for killed requests only
};

// One lane per request: the envelope request into the call's scratch.
hipError_t kread_rewrite_launch(const KreadLaunch &L, hipStream_t stream);
// One wave per (request, span): keystream XORed over the span, gated on the
// request's status word; zeros and the result words for a killed request.
hipError_t kread_ctr_launch(const KreadLaunch &L, hipStream_t stream);
// Behind the key setup of a key table, one wave per stream: zeros over the
// stream's raw record, and over its CtrKey where its key_status is not 0.
hipError_t kread_table_finish_launch(cread::CtrKey *km, const uint32_t *key_status, uint8_t *raw, uint32_t nstreams,
                                     hipStream_t stream);

}  // namespace chip
