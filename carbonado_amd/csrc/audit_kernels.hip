// audit_kernels.hip — KA: slice audits of device-resident bao streams
// (gfx950), the kernels behind include/carbonado_hip_audit.h.
//
// A call is a table of requests (audit_plan.hpp: audit::Req) with prefix
// arrays of work items per request.  Every check of a slice is independent per
// node, as in K5b (bao_tree.hpp: bao_parent_check_kernel): a node re-hashed
// from its STORED bytes equals the CV stored in its own nearest parent (the
// root: the hash), so (request, node) flattens into work items, each finding
// its request by binary search in a prefix array and its node by arithmetic
// from (N, first, last) (audit_nodes.hpp); nothing is tabulated per node and a
// call is a constant number of launches whatever the mix of requests:
//
//  * audit_parent_kernel: one lane per selected parent, b3_parent of its 64
//    stored bytes (K5b's work);
//  * audit_chunk_kernel: one QUAD of lanes per selected chunk (quad_b3.hpp),
//    the hot part.  A chunk is 16 serial compressions; the chunks of an audit
//    are few and scattered (one per request in the usual case: 1024 requests
//    are 1024 chunks).  Lane-per-chunk with the wave staging its 64 chunks
//    through LDS (K3's scheme) needs 64 chunks per wave to fill it and runs
//    each chain at ~700 VALU per compression: 1024 chunks would be 16 waves on
//    a chip of 1024 SIMDs.  A quad runs the chain at ~220 VALU per compression
//    on four times the lanes, and its loads coalesce by themselves: the four
//    lanes read one 64-B block per instruction, all 16 blocks of the chunk in
//    flight before the first compression, so there is nothing to stage but
//    the quad's own 64-B message slot.  (KR's group kernel made the same
//    choice for ragged objects.)  The first chunk's quad checks the header;
//  * audit_content_kernel: behind the verdicts in stream order, 16 B per
//    lane: the verified content of a request whose status stayed 0, zeros
//    otherwise — no unverified byte leaves;
//  * audit_extract_kernel: the proof gather, 16 B per lane (8 for the header),
//    source and destination offsets both computed.
//
// PROOF = false reads a node at its stream offset, PROOF = true at its
// position in the request's packed pre-order; the checks are the same.  A
// workgroup writes only its requests' status words and output ranges.
#include "audit_checks.hpp"
#include "audit_kernels.hpp"

namespace chip {

using namespace bao;

namespace audit {

// BOUND: `total` is a bound the host sized the grid by, not the number of items
// (the device-planned reads, qread_plan.hpp): an item at or past the last
// entry of the prefix array leaves too.
template <bool PROOF, bool BOUND>
__global__ __launch_bounds__(TPB) void audit_parent_kernel(const Req *reqs, const uint64_t *pre, uint32_t nreq,
                                                           uint64_t total, uint32_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total || (BOUND && i >= pre[nreq])) return;
    const uint32_t r = prefix_find(pre, nreq, i);
    const Req a = reqs[r];
    if (!parent_ok<PROOF>(a, i - pre[r])) flag_mismatch(status, r);
}

template <bool PROOF, bool BOUND>
__global__ __launch_bounds__(TPB) void audit_chunk_kernel(const Req *reqs, const uint64_t *pre, uint32_t nreq,
                                                          uint64_t total, uint32_t *status) {
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];  // each quad's message block
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * QUADS + (t >> 2);
    if (i >= total || (BOUND && i >= pre[nreq])) return;  // whole quads leave; the kernel has no workgroup barrier
    const uint32_t r = prefix_find(pre, nreq, i);
    const Req a = reqs[r];
    if (!chunk_ok<PROOF>(a, i - pre[r], msg, t)) flag_mismatch(status, r);
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void audit_content_kernel(const Req *reqs, const uint64_t *pre, uint32_t nreq,
                                                            uint64_t total, const uint32_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const uint32_t r = prefix_find(pre, nreq, i);
    const Req a = reqs[r];
    content_unit<PROOF>(a, UNIT * (i - pre[r]), status[r]);
}

__global__ __launch_bounds__(TPB) void audit_extract_kernel(const Req *reqs, const uint64_t *pre,
                                                            const uint64_t *parents, uint32_t nreq, uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const uint32_t r = prefix_find(pre, nreq, i);
    const Req a = reqs[r];
    uint64_t u = i - pre[r];  // the request's units: the header, 4 per parent, 64 per chunk
    if (u == 0) return proof_header(a);
    u -= 1;
    const uint64_t np = parents[r + 1] - parents[r];
    if (u < 4 * np) return proof_parent_unit(a, u / 4, u % 4);
    u -= 4 * np;
    proof_chunk_unit(a, u / 64, u % 64);
}

}  // namespace audit

hipError_t audit_extract_launch(const AuditLaunch &L, hipStream_t stream) {
    using namespace audit;
    if (L.total_units)
        hipLaunchKernelGGL(audit_extract_kernel, dim3(nblocks(L.total_units, TPB)), dim3(TPB), 0, stream, L.reqs,
                           L.units, L.parents, (uint32_t)L.nreq, L.total_units);
    return hipGetLastError();
}

hipError_t audit_verify_launch(const AuditLaunch &L, hipStream_t stream) {
    using namespace audit;
    const uint32_t nreq = (uint32_t)L.nreq;
    if (L.total_parents) {
        const auto k = L.bounded  ? audit_parent_kernel<false, true>  // (the device-planned reads check streams)
                       : L.proofs ? audit_parent_kernel<true, false>
                                  : audit_parent_kernel<false, false>;
        hipLaunchKernelGGL(k, dim3(nblocks(L.total_parents, TPB)), dim3(TPB), 0, stream, L.reqs, L.parents, nreq,
                           L.total_parents, L.status);
    }
    if (L.total_chunks) {
        const auto k = L.bounded  ? audit_chunk_kernel<false, true>
                       : L.proofs ? audit_chunk_kernel<true, false>
                                  : audit_chunk_kernel<false, false>;
        hipLaunchKernelGGL(k, dim3(nblocks(L.total_chunks, QUADS)), dim3(TPB), 0, stream, L.reqs, L.chunks, nreq,
                           L.total_chunks, L.status);
    }
    if (L.total_units) {  // behind the verdicts, in stream order
        const auto k = L.proofs ? audit_content_kernel<true> : audit_content_kernel<false>;
        hipLaunchKernelGGL(k, dim3(nblocks(L.total_units, TPB)), dim3(TPB), 0, stream, L.reqs, L.units, nreq,
                           L.total_units, L.status);
    }
    return hipGetLastError();
}

}  // namespace chip
