// api_vread.cpp — the vouched ranged reads of include/carbonado_hip_vread.h:
// the ranged reads of api_read.cpp with every rebuilt chunk hashed against the
// CV stored for it in the stream.  The checks and every table are host code in
// read_plan.hpp and vread_plan.hpp; this file uploads the table into the
// caller's scratch and enqueues KA's two checks of the primary slices
// (audit_kernels.hip, one launch each so that parents and chunks flag
// different words), the kernels of vread_kernels.hip and KD's read kernel.
#include "api_read.hpp"
#include "api_vread.hpp"

using namespace chip;
using namespace chip::api;

namespace chip {
namespace api {

int vread_enqueue(vread::Plan &vp, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch, uint32_t flags,
                  void *d_scratch, void *stream) {
    int st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    read::Plan &p = vp.rd;
    CHIP_HIP(h2d(c->stage, scr, p.ka.table.data(), p.ka.table.size(), s));
    VreadLaunch V{};
    V.rd = read_launch_of(p, scr, d_status, d_used);
    V.pathw = reinterpret_cast<uint32_t *>(scr + vp.lay.path);
    V.contra = reinterpret_cast<uint32_t *>(scr + vp.lay.contra);
    V.vouch = d_vouch;
    V.strict = flags & CHIPV_STRICT;
    if (p.nseg) CHIP_HIP(hipMemsetAsync(scr + vp.lay.zero_from(), 0, vp.lay.zero_len(), s));
    return vread_enqueue_launches(V, audit_launch_of(p.ka, scr + p.lay.audit), s);
}

int vread_enqueue_launches(const VreadLaunch &V, AuditLaunch A, hipStream_t s) {
    const ReadLaunch &L = V.rd;
    if (L.nseg) {
        const uint64_t prim_chunks = A.total_chunks;  // KA's checks of every segment's own slice:
        A.total_units = 0;
        A.proofs = false;
        A.total_chunks = 0;  // the parents into the path words,
        A.status = V.pathw;
        CHIP_HIP(audit_verify_launch(A, s));
        A.total_parents = 0; A.total_chunks = prim_chunks;  // the chunks (and the header) into the chunk words
        A.status = L.rstat;
        CHIP_HIP(audit_verify_launch(A, s));
        CHIP_HIP(read_fallback_launch(L, V.pathw, s));
        CHIP_HIP(vread_vouch_launch(V, s));
    }
    CHIP_HIP(vread_finish_launch(V, s));
    CHIP_HIP(read_copy_launch(L, s));
    return CHIP_OK;
}

}  // namespace api
}  // namespace chip

extern "C" {

int chipv_abi_version(void) { return CHIPV_ABI_VERSION; }

uint64_t chipv_read_scratch_len(uint64_t nreq, uint64_t nseg) { return vread::scratch_len(nreq, nseg); }

int chipv_read_ranges_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                          const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                          const uint32_t *req_stream, const uint64_t *start, const uint64_t *len, uint64_t nreq,
                          uint8_t *d_content, const uint64_t *content_off, uint64_t *content_len, uint32_t *d_status,
                          uint32_t *d_used, uint32_t *d_vouch, uint32_t flags, void *d_scratch, uint64_t scratch_len,
                          void *stream) {
    if (nreq == 0) return CHIP_OK;
    vread::Plan vp;
    int st = vread::plan_vread(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len,
                               reinterpret_cast<uintptr_t>(d_hash), padding, chunk_len, nstreams, req_stream, start, len,
                               nreq, reinterpret_cast<uintptr_t>(d_content), content_off, content_len,
                               d_status && d_used && d_vouch, flags, reinterpret_cast<uintptr_t>(d_scratch), scratch_len,
                               &vp);
    if (st != CHIP_OK) return st;
    return vread_enqueue(vp, d_status, d_used, d_vouch, flags, d_scratch, stream);
}

}  // extern "C"
