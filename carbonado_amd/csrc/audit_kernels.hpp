// audit_kernels.hpp — launch interface of audit_kernels.hip (KA) for
// api_audit.cpp.  The table it points to is laid out by audit_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "audit_plan.hpp"

namespace chip {

struct AuditLaunch {
    const audit::Req *reqs;   // device: [nreq]
    const uint64_t *parents;  // device: [nreq + 1] prefix of selected parents per request
    const uint64_t *chunks;   // device: [nreq + 1] prefix of selected chunks per request
    const uint64_t *units;    // device: [nreq + 1] prefix of 16-B gather items per request
    uint64_t nreq, total_parents, total_chunks, total_units;
    bool proofs;              // verify: nodes addressed in the request's proof, not in its stream
    uint32_t *status;         // verify: [nreq], zero at launch
};

// Enqueue the gather of every request's proof (one launch).
hipError_t audit_extract_launch(const AuditLaunch &L, hipStream_t stream);

// Enqueue the checks of every request's parents and chunks, then the content
// gather / zero-fill behind the verdicts (three launches).
hipError_t audit_verify_launch(const AuditLaunch &L, hipStream_t stream);

}  // namespace chip
