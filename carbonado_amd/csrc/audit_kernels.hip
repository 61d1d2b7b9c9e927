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
#include "audit_kernels.hpp"
#include "bao_device.hpp"
#include "chip_internal.hpp"
#include "quad_b3.hpp"

namespace chip {

using namespace bao;

namespace audit {

constexpr int TPB = 256, QUADS = TPB / 4;

// the request of work item i: pre[r] <= i < pre[r + 1] (pre[0] = 0, pre[nreq] > i;
// requests without items are passed over)
__device__ __forceinline__ uint32_t find_req(const uint64_t *pre, uint32_t nreq, uint64_t i) {
    uint32_t lo = 0, hi = nreq;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t hash_word(const uint8_t *h, int w) {  // any alignment
    return (uint32_t)h[4 * w] | (uint32_t)h[4 * w + 1] << 8 | (uint32_t)h[4 * w + 2] << 16 |
           (uint32_t)h[4 * w + 3] << 24;
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void audit_parent_kernel(const Req *reqs, const uint64_t *pre, uint32_t nreq,
                                                           uint64_t total, uint32_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const uint32_t r = find_req(pre, nreq, i);
    const Req a = reqs[r];
    uint64_t s = 0;
    const int lv = parent_item(a.N, a.first, a.last, i - pre[r], &s);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    const uint8_t *node = src + node_off<PROOF>(s, lv, a.N, a.first, a.last);
    uint32_t l[8], rr[8], cv[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const u32x2 x = reinterpret_cast<const u32x2 *>(node)[w];
        const u32x2 y = reinterpret_cast<const u32x2 *>(node + 32)[w];
        l[2 * w] = x.x; l[2 * w + 1] = x.y; rr[2 * w] = y.x; rr[2 * w + 1] = y.y;
    }
    const bool root = is_root(s, lv, a.N);
    b3_parent(l, rr, root, cv);
    bool ok = true;
    if (root) {
        const uint8_t *h = reinterpret_cast<const uint8_t *>(a.hash);
#pragma unroll
        for (int w = 0; w < 8; ++w) ok &= hash_word(h, w) == cv[w];
    } else {
        const uint8_t *slot = src + slot_off<PROOF>(s, lv, a.N, a.first, a.last);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u32x2 x = reinterpret_cast<const u32x2 *>(slot)[w];
            ok &= x.x == cv[2 * w] && x.y == cv[2 * w + 1];
        }
    }
    if (!ok) flag_mismatch(status, r);
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void audit_chunk_kernel(const Req *reqs, const uint64_t *pre, uint32_t nreq,
                                                          uint64_t total, uint32_t *status) {
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];  // each quad's message block
    const int t = threadIdx.x, q = t & 3, g = t >> 2;
    const uint64_t i = (uint64_t)blockIdx.x * QUADS + g;
    if (i >= total) return;  // whole quads leave; the kernel has no workgroup barrier
    const uint32_t r = find_req(pre, nreq, i);
    const Req a = reqs[r];
    const uint64_t c = a.first + (i - pre[r]), N = a.N, n = a.n;
    const uint32_t clen = (uint32_t)chunk_len(c, n);  // n = 0: the empty chunk
    const uint32_t nb = clen == 0 ? 1u : (clen + 63) / 64;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    const uint8_t *cp = src + node_off<PROOF>(c, 0, N, a.first, a.last);
    bool ok = true;
    if (c == a.first && q == 0 && *reinterpret_cast<const uint64_t *>(src) != n) ok = false;  // the header

    const uint32_t slot = (uint32_t)(reinterpret_cast<uintptr_t>(&msg[g][0]) - reinterpret_cast<uintptr_t>(&msg[0][0]));
    const uint8_t *mbase = reinterpret_cast<const uint8_t *>(&msg[0][0]);
    const small::MsgIdx mi(q, slot);
    const uint32_t iv0 = q == 0 ? IV(0) : q == 1 ? IV(1) : q == 2 ? IV(2) : IV(3);
    const uint32_t iv1 = q == 0 ? IV(4) : q == 1 ? IV(5) : q == 2 ? IV(6) : IV(7);
    u32x4 pc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) {  // my 16 B of every block of the chunk, all loads in flight
        const uint32_t off = 64 * b + 16 * q;
        if (off >= clen) pc[b] = u32x4{0u, 0u, 0u, 0u};
        else pc[b] = off + 16 <= clen ? load16_a8(cp + off) : small::load16_bytes(cp + off, clen - off);
    }
    uint32_t h0 = iv0, h1 = iv1;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if ((uint32_t)b < nb) {
            *reinterpret_cast<u32x4 *>(&msg[g][4 * q]) = pc[b];
            wave_sync();
            const bool lastb = (uint32_t)b + 1 == nb;
            const uint32_t flags = (b == 0 ? F_CHUNK_START : 0u) | (lastb ? F_CHUNK_END : 0u) |
                                   (lastb && N == 1 ? F_ROOT : 0u);
            small::compress4(h0, h1, mbase, mi, q, iv0, c, lastb ? clen - 64 * b : 64u, flags);
            wave_sync();
        }
    }
    if (N == 1) {  // the chunk is the root
        const uint8_t *h = reinterpret_cast<const uint8_t *>(a.hash);
        ok &= hash_word(h, q) == h0 && hash_word(h, 4 + q) == h1;
    } else {
        const uint32_t *want = reinterpret_cast<const uint32_t *>(src + slot_off<PROOF>(c, 0, N, a.first, a.last));
        ok &= want[q] == h0 && want[4 + q] == h1;
    }
    if (!ok) flag_mismatch(status, r);
}

template <bool PROOF>
__global__ __launch_bounds__(TPB) void audit_content_kernel(const Req *reqs, const uint64_t *pre, uint32_t nreq,
                                                            uint64_t total, const uint32_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const uint32_t r = find_req(pre, nreq, i);
    const Req a = reqs[r];
    const uint64_t o = UNIT * (i - pre[r]), left = a.olen - o;  // content bytes [o, o + 16) of the request
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.dst) + o;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (status[r] == 0) {  // content starts at the first selected chunk; 16 | 1024: a unit sits in one chunk
        const uint8_t *p = reinterpret_cast<const uint8_t *>(a.src) +
                           node_off<PROOF>(a.first + o / 1024, 0, a.N, a.first, a.last) + o % 1024;
        v = left >= 16 ? load16_a8(p) : load16_partial(p, (uint32_t)left);
    }
    if (left >= 16) *glb(reinterpret_cast<u32x4 *>(dst)) = v;
    else store16_partial(dst, v, (uint32_t)left);
}

__global__ __launch_bounds__(TPB) void audit_extract_kernel(const Req *reqs, const uint64_t *pre,
                                                            const uint64_t *parents, uint32_t nreq, uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const uint32_t r = find_req(pre, nreq, i);
    const Req a = reqs[r];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.dst);
    uint64_t u = i - pre[r];
    if (u == 0) {  // the length header, as stored
        *glb(reinterpret_cast<uint64_t *>(dst)) = *reinterpret_cast<const uint64_t *>(src);
        return;
    }
    u -= 1;
    const uint64_t np = parents[r + 1] - parents[r];
    if (u < 4 * np) {  // 16 B of a parent
        uint64_t s = 0;
        const int lv = parent_item(a.N, a.first, a.last, u / 4, &s);
        const uint64_t w = 16 * (u % 4);
        store16_a8<false>(dst + proof_off(s, lv, a.N, a.first, a.last) + w, load16_a8(src + stream_off(s, lv, a.N) + w));
        return;
    }
    u -= 4 * np;
    const uint64_t c = a.first + u / 64, w = 16 * (u % 64), clen = chunk_len(c, a.n);
    if (w >= clen) return;  // past a short last chunk
    const uint8_t *p = src + stream_off(c, 0, a.N) + w;
    uint8_t *d = dst + proof_off(c, 0, a.N, a.first, a.last) + w;
    if (w + 16 <= clen) store16_a8<false>(d, load16_a8(p));
    else store16_partial(d, load16_partial(p, (uint32_t)(clen - w)), (uint32_t)(clen - w));
}

inline unsigned blocks(uint64_t items, uint64_t per) { return (unsigned)((items + per - 1) / per); }

}  // namespace audit

hipError_t audit_extract_launch(const AuditLaunch &L, hipStream_t stream) {
    using namespace audit;
    if (L.total_units)
        hipLaunchKernelGGL(audit_extract_kernel, dim3(blocks(L.total_units, TPB)), dim3(TPB), 0, stream, L.reqs, L.units,
                           L.parents, (uint32_t)L.nreq, L.total_units);
    return hipGetLastError();
}

hipError_t audit_verify_launch(const AuditLaunch &L, hipStream_t stream) {
    using namespace audit;
    const uint32_t nreq = (uint32_t)L.nreq;
    if (L.total_parents) {
        const auto k = L.proofs ? audit_parent_kernel<true> : audit_parent_kernel<false>;
        hipLaunchKernelGGL(k, dim3(blocks(L.total_parents, TPB)), dim3(TPB), 0, stream, L.reqs, L.parents, nreq,
                           L.total_parents, L.status);
    }
    if (L.total_chunks) {
        const auto k = L.proofs ? audit_chunk_kernel<true> : audit_chunk_kernel<false>;
        hipLaunchKernelGGL(k, dim3(blocks(L.total_chunks, QUADS)), dim3(TPB), 0, stream, L.reqs, L.chunks, nreq,
                           L.total_chunks, L.status);
    }
    if (L.total_units) {  // behind the verdicts, in stream order
        const auto k = L.proofs ? audit_content_kernel<true> : audit_content_kernel<false>;
        hipLaunchKernelGGL(k, dim3(blocks(L.total_units, TPB)), dim3(TPB), 0, stream, L.reqs, L.units, nreq,
                           L.total_units, L.status);
    }
    return hipGetLastError();
}

}  // namespace chip
