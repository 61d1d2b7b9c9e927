// read_kernels.hip — KD: ranged reads of device-resident Zfec|Bao streams that
// survive shard damage (gfx950), the kernels behind
// include/carbonado_hip_read.h that KA does not already supply.
//
// A call is a table of requests cut into segments (read_plan.hpp: read::Req /
// read::Seg; a segment = columns [c0, c1) of one primary shard) and, per
// segment, one slice request of KA over the segment's chunk window of its own
// primary; the same window of the 7 other shards (the fallbacks) is that
// record moved by whole shards.  KA's parent and chunk kernels check the
// primary slices; then
//
//  * read_fallback_parent_kernel / read_fallback_chunk_kernel: KA's checks
//    (audit_checks.hpp) over the fallback slices, GATED: a work item whose
//    segment's primary status word is 0 returns before it loads a node, so an
//    intact read hashes one window per segment and a damaged one eight.  The
//    decision is the device's, there is no synchronisation in the call.  The
//    vouched reads (KV) launch the same pair with PATH set: their gate also
//    reads the segment's path word;
//  * read_resolve_kernel: one lane per request, over its at most 4 segments:
//    8 status words -> direct (own slice authentic), rebuilt (the mask's entry
//    of the host-built table: the four lowest authentic shares and row p of
//    their inverse) or failed; the request's status and used word;
//  * read_kernel: one workgroup per (segment, 4 KiB block of its content), so
//    how the block is served is uniform in the workgroup.  A lane owns the 16
//    bytes of one 16-B-aligned address of the content range; the first and last
//    unit of a segment are partial and written by bytes.  The source column of
//    a unit is not aligned to it: chunk slots are 8-B aligned, so a lane reads
//    two or three aligned 8-B words of the slot and shifts (the four shares of
//    a rebuilt segment sit at the same columns and share the misalignment); a
//    unit whose columns cross into the next chunk slot (parents lie between the
//    slots) is read by bytes.  Rebuilt bytes go through a 1 KiB product table
//    in LDS, entry x = bytes coef[s] * x, s = 0..3, built by the workgroup from
//    the segment's 4 coefficients as repair_decode_kernel builds its own.  A
//    request that failed gets zeros over all its segments.
#include "audit_checks.hpp"
#include "read_device.hpp"
#include "read_kernels.hpp"
#include "zfec_device.hpp"

namespace chip {

using namespace bao;

namespace read {

using audit::QUADS;
using audit::TPB;
static_assert(BLOCK == UNIT * TPB, "content bytes per workgroup");

// items [fpar[g], fpar[g + 1]) are segment g's: 7 x the most parents any of its fallback slices selects
// (BOUND, here and below: `total` or the grid is a bound the host sized the
// launch by, and an item at or past the last prefix entry leaves too)
template <bool PATH, bool BOUND>
__global__ __launch_bounds__(TPB) void read_fallback_parent_kernel(const audit::Req *slices, const Seg *segs,
                                                                   const uint64_t *fpar, uint32_t nseg, uint64_t total,
                                                                   const uint32_t *pathw, uint32_t *rstat) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total || (BOUND && i >= fpar[nseg])) return;
    const uint32_t g = audit::prefix_find(fpar, nseg, i);
    if (own_ok<PATH>(rstat, pathw, g)) return;
    fallback_parent_item(slices, segs, fpar, nseg, i, g, rstat);
}

// items [7 pre[g], 7 pre[g + 1]) are segment g's, pre = KA's chunk prefix of the primary slices
template <bool PATH, bool BOUND>
__global__ __launch_bounds__(TPB) void read_fallback_chunk_kernel(const audit::Req *slices, const Seg *segs,
                                                                  const uint64_t *pre, uint32_t nseg, uint64_t total,
                                                                  const uint32_t *pathw, uint32_t *rstat) {
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];  // each quad's message block
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * QUADS + (t >> 2);
    if (i >= total || (BOUND && i >= FALLBACKS * pre[nseg])) return;  // whole quads leave; no workgroup barrier
    const uint32_t g = audit::prefix_find(pre, nseg, i / FALLBACKS);
    if (own_ok<PATH>(rstat, pathw, g)) return;
    fallback_chunk_item(slices, segs, pre, nseg, i, g, rstat, msg, t);
}

__global__ __launch_bounds__(TPB) void read_resolve_kernel(const Req *reqs, const Seg *segs, const MaskEntry *masks,
                                                           const uint32_t *rstat, uint32_t nreq, uint32_t nseg,
                                                           Served *served, uint32_t *status, uint32_t *used) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r >= nreq) return;
    const Req q = reqs[r];
    uint32_t st = q.status, bits = 0;
    for (uint32_t k = 0; k < q.nseg; ++k) {
        const uint32_t g = q.seg0 + k;
        const Served out = serve_segment<false>(segs, masks, rstat, nullptr, nseg, g);
        if (out.mode == DIRECT) bits |= 1u << segs[g].p;
        else if (out.mode == FAILED) st = CHIP_ERR_ZFEC;
        else
            for (uint32_t s = 0; s < K; ++s) bits |= 1u << (out.sel >> (8 * s) & 0xFFu);
        served[g] = out;
    }
    status[r] = st;
    used[r] = st ? 0u : bits;
}

// Bytes [col, col + nv) of the shard whose chunks start at chunk `ch0` of the
// stream, nv in 1..16, into bytes 0.. of the result.  All of them lie inside
// the shard; they may cross from one chunk slot into the next.
__device__ __forceinline__ u32x4 gather16(const uint8_t *src, uint64_t ch0, uint64_t N, uint32_t col, uint32_t nv) {
    const uint32_t u = col >> 10, w = col & 1023u;
    const uint8_t *p = src + chunk_stream_off(ch0 + u, N) + w;
    if (nv == 16 && w <= 1024 - 16) {  // one slot: aligned 8-B words of it; the third only where it is needed
        const uint32_t m = w & 7u;     // (then it starts before the slot's end, so it lies inside the slot)
        const uint64_t *a = reinterpret_cast<const uint64_t *>(p - m);
        uint64_t x0 = a[0], x1 = a[1];
        if (m) {
            const uint64_t x2 = a[2];
            const uint32_t sh = 8 * m;
            x0 = x0 >> sh | x1 << (64 - sh);
            x1 = x1 >> sh | x2 << (64 - sh);
        }
        return u32x4{(uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32)};
    }
    const uint32_t here = nv < 1024 - w ? nv : 1024 - w;  // bytes of this slot
    const uint8_t *p2 = here < nv ? src + chunk_stream_off(ch0 + u + 1, N) : p;
    uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if ((uint32_t)j < nv) x[j >> 2] |= (uint32_t)((uint32_t)j < here ? p[j] : p2[j - here]) << (8 * (j & 3));
    return u32x4{x[0], x[1], x[2], x[3]};
}

template <bool BOUND>
__global__ __launch_bounds__(TPB) void read_kernel(const Seg *segs, const uint64_t *blocks, uint32_t nseg,
                                                   const Served *served, const uint32_t *status) {
    __shared__ uint32_t tab[256];
    if (BOUND && blockIdx.x >= blocks[nseg]) return;  // the whole workgroup
    const uint32_t g = audit::prefix_find<uint64_t>(blocks, nseg, blockIdx.x);
    const Seg a = segs[g];
    const Served how = served[g];
    const uint32_t mode = status[a.req] ? (uint32_t)FAILED : how.mode;  // uniform in the workgroup
    if (mode == REBUILT) {  // tab[x]: byte s = coef[s] * x
        const uint32_t x = threadIdx.x;
        uint32_t cw = how.coef, acc = 0;
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            if (x >> bit & 1) acc ^= cw;
            cw = zf::gf_double4(cw);
        }
        tab[x] = acc;
        __syncthreads();
    }
    // my unit: the 16-B-aligned addresses [ua, ua + 16) cut to the segment's range [lo, hi)
    const uint64_t end = a.dst + (a.c1 - a.c0);
    const uint64_t ua = a.dst / UNIT * UNIT + UNIT * ((blockIdx.x - blocks[g]) * TPB + threadIdx.x);
    const uint64_t lo = ua > a.dst ? ua : a.dst, hi = ua + UNIT < end ? ua + UNIT : end;
    if (lo >= hi) return;
    const uint32_t nv = (uint32_t)(hi - lo), col = a.c0 + (uint32_t)(lo - a.dst);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    u32x4 out = {0u, 0u, 0u, 0u};
    if (mode == DIRECT) {
        out = gather16(src, (uint64_t)a.p * a.spc, a.N, col, nv);
    } else if (mode == REBUILT) {
        u32x4 v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = gather16(src, (uint64_t)(how.sel >> (8 * s) & 0xFFu) * a.spc, a.N, col, nv);
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t y = tab[zf::comp(v[0], d) >> (8 * b) & 0xFFu] ^
                                   tab[zf::comp(v[1], d) >> (8 * b) & 0xFFu] >> 8 ^
                                   tab[zf::comp(v[2], d) >> (8 * b) & 0xFFu] >> 16 ^
                                   tab[zf::comp(v[3], d) >> (8 * b) & 0xFFu] >> 24;
                word |= (y & 0xFFu) << (8 * b);
            }
            o[d] = word;
        }
        out = u32x4{o[0], o[1], o[2], o[3]};  // (bytes past nv: products of the zeros gather16 left, not stored)
    }
    uint8_t *dst = reinterpret_cast<uint8_t *>(lo);
    if (nv == 16) *glb(reinterpret_cast<u32x4 *>(dst)) = out;  // lo == ua: 16-B aligned
    else store16_partial(dst, out, nv);
}

}  // namespace read

hipError_t read_fallback_launch(const ReadLaunch &L, const uint32_t *pathw, hipStream_t stream) {
    using namespace read;
    const uint32_t nseg = (uint32_t)L.nseg;
    const uint64_t fb_chunks = FALLBACKS * L.prim_chunks;
    if (L.fb_parents) {
        const auto k = L.bounded ? (pathw ? read_fallback_parent_kernel<true, true>
                                          : read_fallback_parent_kernel<false, true>)
                                 : (pathw ? read_fallback_parent_kernel<true, false>
                                          : read_fallback_parent_kernel<false, false>);
        hipLaunchKernelGGL(k, dim3(nblocks(L.fb_parents, TPB)), dim3(TPB), 0, stream, L.slices, L.segs, L.fpar, nseg,
                           L.fb_parents, pathw, L.rstat);
    }
    if (fb_chunks) {
        const auto k = L.bounded ? (pathw ? read_fallback_chunk_kernel<true, true>
                                          : read_fallback_chunk_kernel<false, true>)
                                 : (pathw ? read_fallback_chunk_kernel<true, false>
                                          : read_fallback_chunk_kernel<false, false>);
        hipLaunchKernelGGL(k, dim3(nblocks(fb_chunks, QUADS)), dim3(TPB), 0, stream, L.slices, L.segs, L.chunks, nseg,
                           fb_chunks, pathw, L.rstat);
    }
    return hipGetLastError();
}

hipError_t read_serve_launch(const ReadLaunch &L, hipStream_t stream) {
    using namespace read;
    if (L.nreq)
        hipLaunchKernelGGL(read_resolve_kernel, dim3(nblocks(L.nreq, TPB)), dim3(TPB), 0, stream, L.reqs, L.segs, L.masks,
                           L.rstat, (uint32_t)L.nreq, (uint32_t)L.nseg, L.served, L.status, L.used);
    return read_copy_launch(L, stream);
}

hipError_t read_copy_launch(const ReadLaunch &L, hipStream_t stream) {
    using namespace read;
    if (L.total_blocks)
        hipLaunchKernelGGL(L.bounded ? read_kernel<true> : read_kernel<false>, dim3((unsigned)L.total_blocks),
                           dim3(TPB), 0, stream, L.segs, L.blocks, (uint32_t)L.nseg, L.served, L.status);
    return hipGetLastError();
}

}  // namespace chip
