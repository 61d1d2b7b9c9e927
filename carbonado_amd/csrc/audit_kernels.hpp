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
    bool bounded;             // the totals are bounds: the kernels also read the last prefix entry (streams only)
};

// The launch table of a plan whose uploaded table lies at `base` on the
// device.  The caller sets `proofs` and `status`, and zeroes the totals of the
// launches it leaves out.
inline AuditLaunch audit_launch_of(const audit::Plan &p, const uint8_t *base) {
    AuditLaunch L{};
    L.reqs = reinterpret_cast<const audit::Req *>(base + p.lay.reqs);
    L.parents = reinterpret_cast<const uint64_t *>(base + p.lay.parents);
    L.chunks = reinterpret_cast<const uint64_t *>(base + p.lay.chunks);
    L.units = reinterpret_cast<const uint64_t *>(base + p.lay.units);
    L.nreq = p.nreq;
    L.total_parents = p.total_parents;
    L.total_chunks = p.total_chunks;
    L.total_units = p.total_units;
    return L;
}

// Enqueue the gather of every request's proof (one launch).
hipError_t audit_extract_launch(const AuditLaunch &L, hipStream_t stream);

// Enqueue the checks of every request's parents and chunks, then the content
// gather / zero-fill behind the verdicts (three launches).
hipError_t audit_verify_launch(const AuditLaunch &L, hipStream_t stream);

}  // namespace chip
