// paudit_kernels.hip — KB: slice audits planned on the device (gfx950), the
// kernels behind include/carbonado_hip_paudit.h.
//
// chipa_* plans on the host: it walks the requests, selects every slice, sums
// the work items into prefix arrays and uploads all that; KA's kernels find a
// work item's request by binary search in those arrays.  Here the requests are
// in device memory and every request has the same capacity (P parent slots,
// W chunk slots: paudit_plan.hpp), so a work item finds its request and slot by
// arithmetic on its own index (paudit::item_of, slot-major) and compares the
// slot with the request's own counts; there is no prefix array, no scan and no
// search:
//
//  * paudit_plan_kernel: one lane per request.  The lane loads its stream's
//    record, runs paudit::plan_request (audit::select and audit::req_of, the
//    host plan's own text) and writes its audit::Req and parent count into the
//    scratch, and its status word and lengths where the caller reads them.
//    This is what zeroes the status words (the host-planned calls enqueue a
//    memset);
//  * paudit_parent_kernel: one lane per (request, parent slot j < P); a lane
//    with j at or above the request's parent count leaves, the rest run
//    audit::parent_ok (audit_checks.hpp: KA's check);
//  * paudit_chunk_kernel: one quad per (request, chunk slot k < W) running
//    audit::chunk_ok; whole quads leave, there is no workgroup barrier;
//  * paudit_content_kernel: behind the verdicts in stream order, 16 B per
//    lane over nreq x 64 W units: the verified content of a request whose
//    status stayed 0, zeros otherwise (audit::content_unit, as KA);
//  * paudit_extract_kernel: the proof gather over nreq x (1 + 4 P + 64 W)
//    units, a unit past the request's own counts leaving: the header, 16 B of
//    a parent, 16 B of a chunk (audit::proof_*, as KA).
//
// PROOF = false reads a node at its stream offset, PROOF = true at its
// position in the request's packed pre-order, as in KA.  A lane writes only
// its request's status word and output slot.
#include "audit_checks.hpp"
#include "paudit_kernels.hpp"

namespace chip {

using namespace bao;

namespace paudit {

using audit::QUADS;
using audit::Req;
using audit::TPB;
using audit::UNIT;

__global__ __launch_bounds__(TPB) void paudit_plan_kernel(PauditLaunch L) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r >= L.nreq) return;
    const uint64_t given = L.kind == PROOFS ? L.proof_len[r] : 0;
    const Planned p = plan_request(L.recs, L.shape, L.kind, L.req_stream[r], L.index[r], L.count[r],
                                   L.content + (uint64_t)r * L.content_stride,
                                   L.proofs + (uint64_t)r * L.proof_stride, given);
    L.reqs[r] = p.req;
    L.parents[r] = p.parents;
    L.status[r] = p.status;
    if (L.kind == EXTRACT) L.proof_len[r] = p.proof_len;
    else L.content_len[r] = p.req.olen;
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void paudit_parent_kernel(const Req *reqs, const uint64_t *parents, uint32_t nreq,
                                                            uint64_t total, uint32_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const Item it = item_of(i, nreq, 1);
    if (it.slot >= parents[it.r]) return;
    const Req a = reqs[it.r];
    if (!audit::parent_ok<PROOF>(a, it.slot)) flag_mismatch(status, it.r);
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void paudit_chunk_kernel(const Req *reqs, uint32_t nreq, uint64_t total,
                                                           uint32_t *status) {
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];  // each quad's message block
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * QUADS + (t >> 2);
    if (i >= total) return;  // whole quads leave; the kernel has no workgroup barrier
    const Item it = item_of(i, nreq, 1);
    const Req a = reqs[it.r];
    if (it.slot >= a.last - a.first) return;
    if (!audit::chunk_ok<PROOF>(a, it.slot, msg, t)) flag_mismatch(status, it.r);
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void paudit_content_kernel(const Req *reqs, uint32_t nreq, uint64_t total,
                                                             const uint32_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const Item it = item_of(i, nreq, 64);
    const Req a = reqs[it.r];
    const uint64_t o = 1024 * it.slot + UNIT * it.unit;  // content bytes [o, o + 16) of the request
    if (o >= a.olen) return;
    audit::content_unit<PROOF>(a, o, status[it.r]);
}

__global__ __launch_bounds__(TPB) void paudit_extract_kernel(const Req *reqs, const uint64_t *parents, uint32_t nreq,
                                                             uint64_t P, uint64_t total) {
    uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    if (i < nreq) {  // the length header, as stored
        const Req a = reqs[i];
        if (a.last == a.first) return;  // refused or spare
        return audit::proof_header(a);
    }
    i -= nreq;
    if (i < 4 * P * nreq) {  // 16 B of a parent
        const Item it = item_of(i, nreq, 4);
        if (it.slot >= parents[it.r]) return;
        return audit::proof_parent_unit(reqs[it.r], it.slot, it.unit);
    }
    i -= 4 * P * nreq;
    const Item it = item_of(i, nreq, 64);
    const Req a = reqs[it.r];
    if (it.slot >= a.last - a.first) return;
    audit::proof_chunk_unit(a, it.slot, it.unit);
}

// a grid of at least one workgroup: the number of launches of a call is fixed
inline dim3 grid_of(uint64_t items, uint64_t per) { return dim3(items ? nblocks(items, per) : 1u); }

}  // namespace paudit

hipError_t paudit_verify_launch(const PauditLaunch &L, hipStream_t stream) {
    using namespace paudit;
    const bool proofs = L.kind == PROOFS;
    const uint64_t par = L.P * L.nreq, chk = L.W * L.nreq, units = 64 * chk;  // below 2^36 (paudit::Geometry)
    hipLaunchKernelGGL(paudit_plan_kernel, grid_of(L.nreq, TPB), dim3(TPB), 0, stream, L);
    hipLaunchKernelGGL(proofs ? paudit_parent_kernel<true> : paudit_parent_kernel<false>, grid_of(par, TPB), dim3(TPB),
                       0, stream, L.reqs, L.parents, L.nreq, par, L.status);
    hipLaunchKernelGGL(proofs ? paudit_chunk_kernel<true> : paudit_chunk_kernel<false>, grid_of(chk, QUADS), dim3(TPB),
                       0, stream, L.reqs, L.nreq, chk, L.status);
    hipLaunchKernelGGL(proofs ? paudit_content_kernel<true> : paudit_content_kernel<false>, grid_of(units, TPB),
                       dim3(TPB), 0, stream, L.reqs, L.nreq, units, L.status);
    return hipGetLastError();
}

hipError_t paudit_extract_launch(const PauditLaunch &L, hipStream_t stream) {
    using namespace paudit;
    const uint64_t units = extract_items(L.nreq, L.P, L.W);
    hipLaunchKernelGGL(paudit_plan_kernel, grid_of(L.nreq, TPB), dim3(TPB), 0, stream, L);
    hipLaunchKernelGGL(paudit_extract_kernel, grid_of(units, TPB), dim3(TPB), 0, stream, L.reqs, L.parents, L.nreq,
                       L.P, units);
    return hipGetLastError();
}

}  // namespace chip
