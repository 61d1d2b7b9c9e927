// paudit_kernels.hpp — launch interface of paudit_kernels.hip (KB) for
// api_paudit.cpp.  The scratch it points to is laid out by paudit_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "paudit_plan.hpp"

namespace chip {

struct PauditLaunch {
    const paudit::StreamRec *recs;  // device: the stream table's or the root table's records
    paudit::Shape shape;
    paudit::Kind kind;
    const uint32_t *req_stream;     // device: [nreq]
    const uint64_t *index, *count;  // device: [nreq]
    uint32_t nreq;
    uint64_t W, P;                  // chunk and parent slots per request (paudit::Geometry)
    uint64_t content, content_stride;  // address of slot 0 and the slots' pitch (VERIFY, PROOFS)
    uint64_t proofs, proof_stride;     // (EXTRACT, PROOFS)
    uint64_t *content_len;          // device: [nreq], written (VERIFY, PROOFS)
    uint64_t *proof_len;            // device: [nreq], written (EXTRACT), read (PROOFS)
    uint32_t *status;               // device: [nreq], written
    audit::Req *reqs;               // scratch: [nreq]
    uint64_t *parents;              // scratch: [nreq] selected parents per request
};

// Enqueue the plan, the parent check, the chunk check and the content gather /
// zero-fill of a verify call (four launches); kind is VERIFY or PROOFS.
hipError_t paudit_verify_launch(const PauditLaunch &L, hipStream_t stream);

// Enqueue the plan and the proof gather of an extract call (two launches).
hipError_t paudit_extract_launch(const PauditLaunch &L, hipStream_t stream);

}  // namespace chip
