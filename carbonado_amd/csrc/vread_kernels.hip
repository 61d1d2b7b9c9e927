// vread_kernels.hip — KV: vouched ranged reads (gfx950), the kernels behind
// include/carbonado_hip_vread.h that KA and KD do not already supply.
//
// A call is the table of a ranged read (read_plan.hpp) and two more words per
// segment.  KA's parent kernel checks the primary slices into the PATH word of
// each segment, KA's chunk kernel into its CHUNK word (rstat[g], where KD keeps
// its one word); a slice is authentic when both are 0.  Then
//
//  * KD's gated checks of the 7 fallback slices (read_kernels.hip:
//    read_fallback_parent_kernel / read_fallback_chunk_kernel), launched with
//    the gate that reads "either word set";
//  * vread_resolve_kernel: one lane per segment: direct, rebuilt or failed, by
//    KD's own decision (read_device.hpp: serve_segment);
//  * vread_vouch_kernel, the new hot part: one QUAD of lanes per (segment,
//    window chunk), found through KA's chunk prefix of the primary slices.
//    GATED on the segment: only mode REBUILT under a path word of 0 runs; every
//    other quad returns before it loads a byte of a stream, so an intact call
//    pays the launch and no hashing.  The quad runs chunk_ok's chain
//    (quad_b3.hpp; all chunks are full, the counter is p spc + c, never the
//    root) over message blocks that exist only in registers and the quad's
//    64-B LDS slot: block b of the rebuilt chunk is sum_s coef[s] * share
//    sel[s] at the same 64 bytes of the four shares' chunk slots.  A lane
//    loads its 16 B of 4 blocks of the 4 shares (16 loads in flight), combines
//    and compresses them, four times.  The product is the packed double-and-add
//    of zf::gf_double4 in Horner form over the coefficient bits,
//    acc = 2 acc ^ sum_s (bit k of coef[s] ? x[s] : 0), k = 7..0: 7 doublings
//    and 32 masked XORs per word of four bytes whatever the four coefficients
//    are, no table, so the 64 quads of a workgroup may belong to 64 segments
//    with different coefficients at no cost in LDS.  The 32 masks are made
//    once per quad.  The CV is compared with the one stored in the chunk's
//    nearest parent, which the path word vouches for; a mismatch flags the
//    segment's contradiction word;
//  * vread_finish_kernel: one lane per request over its segments' classes:
//    status, used and vouch.  It runs before KD's read kernel, which reads the
//    final status.
#include "audit_checks.hpp"
#include "read_device.hpp"
#include "vread_kernels.hpp"
#include "zfec_device.hpp"

namespace chip {

using namespace bao;

namespace vread {

using audit::QUADS;
using audit::TPB;
using read::K;
using read::M;

__global__ __launch_bounds__(TPB) void vread_resolve_kernel(const read::Seg *segs, const read::MaskEntry *masks,
                                                            const uint32_t *rstat, const uint32_t *pathw, uint32_t nseg,
                                                            read::Served *served) {
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    if (g >= nseg) return;
    served[g] = read::serve_segment<true>(segs, masks, rstat, pathw, nseg, g);
}

// sum_s coef[s] * x[s] on four packed bytes; mk[s][k] = all ones where bit k of coef[s] is set
__device__ __forceinline__ uint32_t gf_comb4(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3,
                                             const uint32_t (&mk)[4][8]) {
    uint32_t acc = (x0 & mk[0][7]) ^ (x1 & mk[1][7]) ^ (x2 & mk[2][7]) ^ (x3 & mk[3][7]);
#pragma unroll
    for (int k = 6; k >= 0; --k)
        acc = zf::gf_double4(acc) ^ (x0 & mk[0][k]) ^ (x1 & mk[1][k]) ^ (x2 & mk[2][k]) ^ (x3 & mk[3][k]);
    return acc;
}

// items [pre[g], pre[g + 1]) are segment g's window chunks, pre = KA's chunk prefix of the primary slices
// (BOUND: `total` is a bound the host sized the grid by; an item at or past pre[nseg] leaves too)
template <bool BOUND>
__global__ __launch_bounds__(TPB) void vread_vouch_kernel(const audit::Req *slices, const uint64_t *pre, uint32_t nseg,
                                                          uint64_t total, const read::Served *served,
                                                          const uint32_t *pathw, uint32_t *contra) {
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];  // each quad's message block
    const int t = threadIdx.x, q = t & 3, qd = t >> 2;
    const uint64_t i = (uint64_t)blockIdx.x * QUADS + qd;
    if (i >= total || (BOUND && i >= pre[nseg])) return;  // whole quads leave; the kernel has no workgroup barrier
    const uint32_t g = audit::prefix_find(pre, nseg, i);
    const read::Served how = served[g];
    if (how.mode != read::REBUILT || pathw[g] != 0) return;  // nothing to vouch for, or nothing to compare with
    const audit::Req a = slices[g];
    const uint64_t N = a.N, spc = N / M;
    const uint64_t c = a.first + (i - pre[g]);  // the chunk of the stream that is rebuilt
    const uint64_t u = c % spc;                 // its place in a shard
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    const uint8_t *cp[4];
    uint32_t mk[4][8];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint64_t shard = how.sel >> (8 * s) & 0xFFu;
        cp[s] = src + audit::stream_off(shard * spc + u, 0, N) + 16 * q;
        const uint32_t cf = how.coef >> (8 * s) & 0xFFu;
#pragma unroll
        for (int k = 0; k < 8; ++k) mk[s][k] = 0u - (cf >> k & 1u);
    }
    const uint32_t slot = (uint32_t)(reinterpret_cast<uintptr_t>(&msg[qd][0]) - reinterpret_cast<uintptr_t>(&msg[0][0]));
    const uint8_t *mbase = reinterpret_cast<const uint8_t *>(&msg[0][0]);
    const small::MsgIdx mi(q, slot);
    const uint32_t iv0 = q == 0 ? IV(0) : q == 1 ? IV(1) : q == 2 ? IV(2) : IV(3);
    const uint32_t iv1 = q == 0 ? IV(4) : q == 1 ? IV(5) : q == 2 ? IV(6) : IV(7);
    uint32_t h0 = iv0, h1 = iv1;
#pragma unroll
    for (int grp = 0; grp < 4; ++grp) {
        u32x4 v[4][4];  // my 16 B of blocks 4 grp .. 4 grp + 3 of the four shares, all loads in flight
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s) v[b][s] = load16_a8(cp[s] + 64 * (4 * grp + b));
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            u32x4 m;
            m.x = gf_comb4(v[b][0].x, v[b][1].x, v[b][2].x, v[b][3].x, mk);
            m.y = gf_comb4(v[b][0].y, v[b][1].y, v[b][2].y, v[b][3].y, mk);
            m.z = gf_comb4(v[b][0].z, v[b][1].z, v[b][2].z, v[b][3].z, mk);
            m.w = gf_comb4(v[b][0].w, v[b][1].w, v[b][2].w, v[b][3].w, mk);
            *reinterpret_cast<u32x4 *>(&msg[qd][4 * q]) = m;
            wave_sync();
            const int blk = 4 * grp + b;
            const uint32_t flags = (blk == 0 ? F_CHUNK_START : 0u) | (blk == 15 ? F_CHUNK_END : 0u);
            small::compress4(h0, h1, mbase, mi, q, iv0, c, 64u, flags);
            wave_sync();
        }
    }
    const uint32_t *want = reinterpret_cast<const uint32_t *>(src + audit::slot_off<false>(c, 0, N, a.first, a.last));
    if (want[q] != h0 || want[4 + q] != h1) flag_mismatch(contra, g);
}

// PLANNED (the device-planned reads, qread_kernels.hip): a request the plan
// refused keeps the plan's status, which can be 1 there; the host plan's only
// refusal is 7, which `failed` gives.
template <bool PLANNED>
__global__ __launch_bounds__(TPB) void vread_finish_kernel(const read::Req *reqs, const read::Seg *segs,
                                                           const read::Served *served, const uint32_t *pathw,
                                                           const uint32_t *contra, uint32_t nreq, uint32_t strict,
                                                           uint32_t *status, uint32_t *used, uint32_t *vouch) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r >= nreq) return;
    const read::Req rq = reqs[r];
    uint32_t bits = 0, v = 0;
    bool failed = rq.status != 0;
    for (uint32_t k = 0; k < rq.nseg; ++k) {
        const uint32_t g = rq.seg0 + k;
        const read::Served how = served[g];
        if (how.mode == read::DIRECT) {
            bits |= 1u << segs[g].p;
        } else if (how.mode == read::FAILED) {
            failed = true;
        } else {
            for (uint32_t s = 0; s < K; ++s) bits |= 1u << (how.sel >> (8 * s) & 0xFFu);
            v |= pathw[g] ? CHIPV_UNVOUCHED : contra[g] ? CHIPV_CONTRADICTED : CHIPV_VOUCHED;
        }
    }
    const uint32_t st = PLANNED && rq.status                          ? rq.status  // refused by the plan: no segment
                        : v & CHIPV_CONTRADICTED                      ? (uint32_t)CHIP_ERR_BAO_HASH_MISMATCH
                        : failed || (strict && (v & CHIPV_UNVOUCHED)) ? (uint32_t)CHIP_ERR_ZFEC
                                                                      : 0u;
    status[r] = st;
    used[r] = st ? 0u : bits;
    vouch[r] = v;
}

}  // namespace vread

hipError_t vread_vouch_launch(const VreadLaunch &L, hipStream_t stream) {
    using namespace vread;
    const ReadLaunch &R = L.rd;
    const uint32_t nseg = (uint32_t)R.nseg;
    if (nseg)
        hipLaunchKernelGGL(vread_resolve_kernel, dim3(nblocks(nseg, TPB)), dim3(TPB), 0, stream, R.segs, R.masks,
                           R.rstat, L.pathw, nseg, R.served);
    if (R.prim_chunks)
        hipLaunchKernelGGL(R.bounded ? vread_vouch_kernel<true> : vread_vouch_kernel<false>,
                           dim3(nblocks(R.prim_chunks, QUADS)), dim3(TPB), 0, stream, R.slices, R.chunks, nseg,
                           R.prim_chunks, R.served, L.pathw, L.contra);
    return hipGetLastError();
}

hipError_t vread_finish_launch(const VreadLaunch &L, hipStream_t stream) {
    using namespace vread;
    const ReadLaunch &R = L.rd;
    if (R.nreq)
        hipLaunchKernelGGL(R.bounded ? vread_finish_kernel<true> : vread_finish_kernel<false>,
                           dim3(nblocks(R.nreq, TPB)), dim3(TPB), 0, stream, R.reqs, R.segs, R.served, L.pathw, L.contra,
                           (uint32_t)R.nreq, L.strict, R.status, R.used, L.vouch);
    return hipGetLastError();
}

}  // namespace chip
