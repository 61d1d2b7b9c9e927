// api_audit.cpp — the slice audits of include/carbonado_hip_audit.h: batched
// extract_slice / verify_slice over device-resident streams, and verify_slice
// from extracted proofs.  The checks, the layout and the per-request table are
// host code in audit_plan.hpp; this file uploads the table into the caller's
// scratch and enqueues the kernels of audit_kernels.hip behind it.
#include "api_common.hpp"
#include "audit_kernels.hpp"

using namespace chip;
using namespace chip::api;

namespace {

// the table into d_scratch on s (through the thread's pinned ring: the host
// copy may go once this returns), then the kernels
int enqueue(audit::Plan &p, bool verify, bool proofs, uint32_t *d_status, void *d_scratch, hipStream_t s) {
    Ctx *c;
    int st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    CHIP_HIP(h2d(c->stage, scr, p.table.data(), p.table.size(), s));
    AuditLaunch L = audit_launch_of(p, scr);
    L.proofs = proofs;
    L.status = d_status;
    if (verify) {
        CHIP_HIP(hipMemsetAsync(d_status, 0, p.nreq * sizeof(uint32_t), s));
        CHIP_HIP(audit_verify_launch(L, s));
    } else {
        CHIP_HIP(audit_extract_launch(L, s));
    }
    return CHIP_OK;
}

}  // namespace

extern "C" {

int chipa_abi_version(void) { return CHIPA_ABI_VERSION; }

int chipa_slice_layout(const uint64_t *content_len, const uint64_t *index, const uint64_t *count, uint64_t nreq,
                       uint64_t align, uint64_t *proof_off, uint64_t *proof_len, uint64_t *content_off,
                       uint64_t *content_len_out, uint64_t *proof_total, uint64_t *content_total) {
    return audit::layout(content_len, index, count, nreq, align, proof_off, proof_len, content_off, content_len_out,
                         proof_total, content_total);
}

uint64_t chipa_audit_scratch_len(uint64_t nstreams, uint64_t nreq) { return audit::scratch_len(nstreams, nreq); }

int chipa_extract_slices_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                             uint64_t nstreams, const uint32_t *req_stream, const uint64_t *index,
                             const uint64_t *count, uint64_t nreq, uint8_t *d_proofs, const uint64_t *proof_off,
                             const uint64_t *proof_len, void *d_scratch, void *stream) {
    if (nreq == 0) return CHIP_OK;
    if (!d_scratch || misaligned16(d_scratch)) return CHIP_ERR_INVALID_ARG;
    audit::Plan p;
    int st = audit::plan_extract(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len, nstreams, req_stream, index,
                                 count, nreq, reinterpret_cast<uintptr_t>(d_proofs), proof_off, proof_len, &p);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    return enqueue(p, false, false, nullptr, d_scratch, static_cast<hipStream_t>(stream));
}

int chipa_verify_slices_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                            const uint8_t *d_hash, uint64_t nstreams, const uint32_t *req_stream,
                            const uint64_t *index, const uint64_t *count, uint64_t nreq, uint8_t *d_content,
                            const uint64_t *content_off, uint64_t *content_len, uint32_t *d_status, void *d_scratch,
                            void *stream) {
    if (nreq == 0) return CHIP_OK;
    audit::Plan p;
    int st = audit::plan_verify(false, reinterpret_cast<uintptr_t>(d_streams), in_off, in_len, nstreams, req_stream,
                                nullptr, reinterpret_cast<uintptr_t>(d_hash), index, count, nreq,
                                reinterpret_cast<uintptr_t>(d_content), content_off, content_len,
                                d_status && d_scratch && !misaligned16(d_scratch), &p);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    return enqueue(p, true, false, d_status, d_scratch, static_cast<hipStream_t>(stream));
}

int chipa_verify_proofs_dev(const uint8_t *d_proofs, const uint64_t *proof_off, const uint64_t *proof_len,
                            const uint64_t *content_len, const uint8_t *d_hash, const uint64_t *index,
                            const uint64_t *count, uint64_t nreq, uint8_t *d_content, const uint64_t *content_off,
                            uint64_t *content_len_out, uint32_t *d_status, void *d_scratch, void *stream) {
    if (nreq == 0) return CHIP_OK;
    audit::Plan p;
    int st = audit::plan_verify(true, reinterpret_cast<uintptr_t>(d_proofs), proof_off, proof_len, nreq, nullptr,
                                content_len, reinterpret_cast<uintptr_t>(d_hash), index, count, nreq,
                                reinterpret_cast<uintptr_t>(d_content), content_off, content_len_out,
                                d_status && d_scratch && !misaligned16(d_scratch), &p);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    return enqueue(p, true, true, d_status, d_scratch, static_cast<hipStream_t>(stream));
}

}  // extern "C"
