// api_read.cpp — the ranged reads of include/carbonado_hip_read.h: byte ranges
// of device-resident Zfec|Bao objects, rebuilt from other shards where the
// primary's chunks are damaged.  The checks, the layout, the segments and
// every table are host code in read_plan.hpp; this file uploads the table into
// the caller's scratch and enqueues KA's checks of the primary slices
// (audit_kernels.hip) and the kernels of read_kernels.hip behind it.
#include "api_read.hpp"

using namespace chip;
using namespace chip::api;

namespace chip {
namespace api {

int read_enqueue_launches(const ReadLaunch &L, AuditLaunch A, hipStream_t s) {
    if (L.nseg) {
        A.total_units = 0;  // KA's checks of every segment's own slice
        A.proofs = false;
        A.status = L.rstat;
        CHIP_HIP(audit_verify_launch(A, s));
        CHIP_HIP(read_fallback_launch(L, nullptr, s));
    }
    CHIP_HIP(read_serve_launch(L, s));
    return CHIP_OK;
}

}  // namespace api
}  // namespace chip

extern "C" {

int chipd_abi_version(void) { return CHIPD_ABI_VERSION; }

int chipd_read_layout(const uint32_t *chunk_len, const uint32_t *padding, uint64_t nstreams, const uint32_t *req_stream,
                      const uint64_t *start, const uint64_t *len, uint64_t nreq, uint64_t align, uint64_t *content_off,
                      uint64_t *content_len, uint64_t *content_total, uint64_t *nseg) {
    return read::layout(chunk_len, padding, nstreams, req_stream, start, len, nreq, align, content_off, content_len,
                        content_total, nseg);
}

uint64_t chipd_read_scratch_len(uint64_t nreq, uint64_t nseg) { return read::scratch_len(nreq, nseg); }

int chipd_read_ranges_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                          const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                          const uint32_t *req_stream, const uint64_t *start, const uint64_t *len, uint64_t nreq,
                          uint8_t *d_content, const uint64_t *content_off, uint64_t *content_len, uint32_t *d_status,
                          uint32_t *d_used, void *d_scratch, uint64_t scratch_len, void *stream) {
    if (nreq == 0) return CHIP_OK;
    read::Plan p;
    int st = read::plan_read(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len, reinterpret_cast<uintptr_t>(d_hash),
                             padding, chunk_len, nstreams, req_stream, start, len, nreq,
                             reinterpret_cast<uintptr_t>(d_content), content_off, content_len, d_status && d_used,
                             reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &p);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    CHIP_HIP(h2d(c->stage, scr, p.ka.table.data(), p.ka.table.size(), s));
    const ReadLaunch L = read_launch_of(p, scr, d_status, d_used);
    if (p.nseg) CHIP_HIP(hipMemsetAsync(L.rstat, 0, read::M * p.nseg * sizeof(uint32_t), s));
    return read_enqueue_launches(L, audit_launch_of(p.ka, scr + p.lay.audit), s);
}

}  // extern "C"
