// api_paudit.cpp — the device-planned slice audits of
// include/carbonado_hip_paudit.h.  chipp_root_table_dev is the auditor's one
// upload (paudit_plan.hpp: the checks and the table).  The three calls do O(1)
// host work (paudit::plan_call), fill KB's launch table with pointers into the
// caller's buffers and their own scratch, and enqueue the kernels of
// paudit_kernels.hip.  Kernels only: no upload, no memset, no synchronisation,
// no allocation after the thread's first call.
#include "api_common.hpp"
#include "paudit_kernels.hpp"

using namespace chip;
using namespace chip::api;

namespace {

struct Call {
    paudit::Kind kind;
    const void *d_table;
    bool have_info;
    uint64_t nstreams, max_chunks;
    const uint32_t *d_req_stream;
    const uint64_t *d_index, *d_count;
    uint64_t nreq, max_count;
    uint8_t *d_content;
    uint64_t content_stride;
    uint64_t *d_content_len;
    uint8_t *d_proofs;
    uint64_t proof_stride;
    uint64_t *d_proof_len;
    uint32_t *d_status;
    void *d_scratch;
    uint64_t scratch_len;
    void *stream;
};

int audit_planned(const Call &a) {
    if (a.nreq == 0) return CHIP_OK;
    const bool with_content = a.kind != paudit::EXTRACT, with_proofs = a.kind != paudit::VERIFY;
    const bool have = a.d_table && a.have_info && a.d_req_stream && a.d_index && a.d_count && a.d_status &&
                      a.d_scratch && (!with_content || (a.d_content && a.d_content_len)) &&
                      (!with_proofs || (a.d_proofs && a.d_proof_len));
    paudit::Geometry g;
    paudit::ScratchLayout lay;
    int st = paudit::plan_call(have, reinterpret_cast<uintptr_t>(a.d_table), a.max_chunks, a.nreq, a.max_count,
                               with_content, reinterpret_cast<uintptr_t>(a.d_content), a.content_stride, with_proofs,
                               reinterpret_cast<uintptr_t>(a.d_proofs), a.proof_stride,
                               reinterpret_cast<uintptr_t>(a.d_scratch), a.scratch_len, &g, &lay);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    uint8_t *scr = static_cast<uint8_t *>(a.d_scratch);

    PauditLaunch L{};
    L.recs = static_cast<const paudit::StreamRec *>(a.d_table);
    L.shape = paudit::Shape{a.nstreams, a.max_chunks, a.max_count};
    L.kind = a.kind;
    L.req_stream = a.d_req_stream; L.index = a.d_index; L.count = a.d_count;
    L.nreq = (uint32_t)a.nreq;
    L.W = g.W; L.P = g.P;
    L.content = reinterpret_cast<uint64_t>(a.d_content); L.content_stride = a.content_stride;
    L.proofs = reinterpret_cast<uint64_t>(a.d_proofs); L.proof_stride = a.proof_stride;
    L.content_len = a.d_content_len;
    L.proof_len = a.d_proof_len;
    L.status = a.d_status;
    L.reqs = reinterpret_cast<audit::Req *>(scr + lay.reqs);
    L.parents = reinterpret_cast<uint64_t *>(scr + lay.parents);
    CHIP_HIP(a.kind == paudit::EXTRACT ? paudit_extract_launch(L, s) : paudit_verify_launch(L, s));
    return CHIP_OK;
}

}  // namespace

extern "C" {

int chipp_abi_version(void) { return CHIPP_ABI_VERSION; }

uint64_t chipp_root_table_len(uint64_t nroots) { return paudit::root_table_len(nroots); }

int chipp_root_table_dev(const uint64_t *content_len, const uint8_t *d_hash, uint64_t nroots, void *d_table,
                         uint64_t table_len, chipp_root_info *info, void *stream) {
    std::vector<uint8_t> table;
    chipp_root_info out;
    int st = paudit::plan_root_table(content_len, reinterpret_cast<uintptr_t>(d_hash), nroots,
                                     reinterpret_cast<uintptr_t>(d_table), table_len, info ? &out : nullptr, &table);
    if (info) std::memset(info, 0, sizeof *info);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    if (!table.empty()) CHIP_HIP(h2d(c->stage, d_table, table.data(), table.size(), static_cast<hipStream_t>(stream)));
    *info = out;
    return CHIP_OK;
}

uint64_t chipp_audit_scratch_len(uint64_t info_max_chunks, uint64_t nreq, uint64_t max_count) {
    return paudit::scratch_len(info_max_chunks, nreq, max_count);
}

uint64_t chipp_proof_bound(uint64_t max_chunks, uint64_t max_count) {
    return paudit::proof_bound(max_chunks, max_count);
}

int chipp_verify_slices_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                            const uint64_t *d_index, const uint64_t *d_count, uint64_t nreq, uint64_t max_count,
                            uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len, uint32_t *d_status,
                            void *d_scratch, uint64_t scratch_len, void *stream) {
    return audit_planned(Call{paudit::VERIFY, d_table, info != nullptr, info ? info->nstreams : 0,
                              info ? info->max_chunks : 0, d_req_stream, d_index, d_count, nreq, max_count, d_content,
                              content_stride, d_content_len, nullptr, 0, nullptr, d_status, d_scratch, scratch_len,
                              stream});
}

int chipp_extract_slices_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                             const uint64_t *d_index, const uint64_t *d_count, uint64_t nreq, uint64_t max_count,
                             uint8_t *d_proofs, uint64_t proof_stride, uint64_t *d_proof_len, uint32_t *d_status,
                             void *d_scratch, uint64_t scratch_len, void *stream) {
    return audit_planned(Call{paudit::EXTRACT, d_table, info != nullptr, info ? info->nstreams : 0,
                              info ? info->max_chunks : 0, d_req_stream, d_index, d_count, nreq, max_count, nullptr, 0,
                              nullptr, d_proofs, proof_stride, d_proof_len, d_status, d_scratch, scratch_len, stream});
}

int chipp_verify_proofs_dev(const void *d_roots, const chipp_root_info *root_info, const uint32_t *d_req_stream,
                            const uint64_t *d_index, const uint64_t *d_count, uint64_t nreq, uint64_t max_count,
                            const uint8_t *d_proofs, uint64_t proof_stride, const uint64_t *d_proof_len,
                            uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len, uint32_t *d_status,
                            void *d_scratch, uint64_t scratch_len, void *stream) {
    return audit_planned(Call{paudit::PROOFS, d_roots, root_info != nullptr, root_info ? root_info->nroots : 0,
                              root_info ? root_info->max_chunks : 0, d_req_stream, d_index, d_count, nreq, max_count,
                              d_content, content_stride, d_content_len, const_cast<uint8_t *>(d_proofs), proof_stride,
                              const_cast<uint64_t *>(d_proof_len), d_status, d_scratch, scratch_len, stream});
}

}  // extern "C"
