// qread_kernels.hip — KQ: the plan of a ranged read made on the device
// (gfx950), the kernels behind include/carbonado_hip_qread.h that KA, KD and KV
// do not already supply.
//
// chipd_read_ranges_dev plans on the host: it walks the requests, cuts them
// into segments, selects every segment's slice, sums the work items into
// prefix arrays and uploads all that.  Here the requests are in device memory
// and the same tables are written where the other kernels read them:
//
//  * qread_request_kernel: one lane per request.  The lane loads its stream's
//    record, runs read::range_of and read::cut_segment (qread_device.hpp: the
//    host plan's own text), and writes its read::Req, its S segment slots
//    (read::Seg, the slice request of KA) and the four work-item COUNTS of
//    every slot: parents, chunks, fallback parents, read blocks.  Unused slots
//    count zero.  It also zeroes its slots' status words, which the checks
//    behind it flag (the host-planned calls enqueue a memset for that; here
//    the call enqueues kernels only).  A few hundred bytes of stores per lane,
//    no loop over data;
//  * the exclusive scan of the four count arrays (S nreq + 1 entries of 64
//    bits each) in place, in the three-launch form: qread_scan_tile_kernel scans
//    a tile of 1024 entries per workgroup (4 per lane, a shuffle scan across
//    the wave, the 4 wave totals through LDS) and writes the tile's total;
//    qread_scan_sums_kernel, one workgroup per array, scans the tile totals
//    (looping with a carry); qread_scan_add_kernel adds a tile's offset.  No
//    workgroup waits on another: the order is the stream's.
//
// Arrays of a call are a few thousand to a few hundred thousand entries, so
// the scan is launch-bound; the three launches are what a call pays for not
// touching the host.
#include "audit_checks.hpp"
#include "qread_kernels.hpp"

namespace chip {

using namespace bao;

namespace qread {

using audit::TPB;
constexpr int PER_LANE = 4;
constexpr int WAVES = TPB / 64;
static_assert(SCAN_TILE == (uint64_t)TPB * PER_LANE, "entries per workgroup");

__global__ __launch_bounds__(TPB) void qread_request_kernel(const StreamRec *recs, Shape sh, const uint32_t *req_stream,
                                                            const uint64_t *start, const uint64_t *len, uint32_t nreq,
                                                            uint64_t content, uint64_t stride, Tables t,
                                                            uint32_t *rstat, uint32_t *pathw, uint32_t *contra) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r >= nreq) return;
    plan_request(recs, sh, r, req_stream[r], start[r], len[r], content + (uint64_t)r * stride, t);
    // the status words of my slots, zero for the checks behind (the host-planned calls enqueue a memset for this)
    const uint64_t nslot = (uint64_t)nreq * sh.S;
    for (uint32_t k = 0; k < sh.S; ++k) {
        const uint64_t g = (uint64_t)r * sh.S + k;
        rstat[g] = 0;
        for (uint32_t j = 0; j < read::FALLBACKS; ++j) rstat[nslot + read::FALLBACKS * g + j] = 0;
        if (pathw) {
            pathw[g] = 0;
            contra[g] = 0;
        }
    }
    if (r == nreq - 1) {  // the entry behind the last slot: the scan leaves the total there
        const uint64_t end = (uint64_t)nreq * sh.S;
        t.parents[end] = 0; t.chunks[end] = 0; t.fpar[end] = 0; t.blocks[end] = 0;
    }
}

// Exclusive scan of x across the workgroup's lanes in lane order; *total = the sum.
__device__ __forceinline__ uint64_t block_exclusive(uint64_t x, uint64_t (&wsum)[WAVES], uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    __syncthreads();  // wsum is reused by the caller's next round
    *total = all;
    return before + inc - x;
}

// grid (tiles, arrays): array a = base + a pitch, n entries each
__global__ __launch_bounds__(TPB) void qread_scan_tile_kernel(uint64_t *base, uint64_t pitch, uint64_t n,
                                                              uint64_t *sums) {
    __shared__ uint64_t wsum[WAVES];
    uint64_t *arr = base + blockIdx.y * pitch;
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * PER_LANE;
    uint64_t v[PER_LANE], mine = 0;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        v[j] = i0 + j < n ? arr[i0 + j] : 0;
        mine += v[j];
    }
    uint64_t total;
    uint64_t run = block_exclusive(mine, wsum, &total);
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        if (i0 + j < n) arr[i0 + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// grid (arrays): the `tiles` tile totals of array a, scanned in place
__global__ __launch_bounds__(TPB) void qread_scan_sums_kernel(uint64_t *sums, uint64_t tiles) {
    __shared__ uint64_t wsum[WAVES];
    uint64_t *arr = sums + (uint64_t)blockIdx.x * tiles;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < tiles; b += TPB) {  // uniform trip count: every lane meets the barriers
        const uint64_t i = b + threadIdx.x;
        const uint64_t x = i < tiles ? arr[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive(x, wsum, &total);
        if (i < tiles) arr[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(TPB) void qread_scan_add_kernel(uint64_t *base, uint64_t pitch, uint64_t n,
                                                             const uint64_t *sums) {
    if (blockIdx.x == 0) return;  // the first tile's offset is 0
    uint64_t *arr = base + blockIdx.y * pitch;
    const uint64_t off = sums[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x];
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * PER_LANE;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j)
        if (i0 + j < n) arr[i0 + j] += off;
}

}  // namespace qread

hipError_t qread_plan_launch(const QreadLaunch &L, hipStream_t stream) {
    using namespace qread;
    const uint64_t n = L.nreq * L.shape.S + 1;
    const dim3 tiles((unsigned)L.scan_blocks, SCAN_ARRAYS);
    hipLaunchKernelGGL(qread_request_kernel, dim3(nblocks(L.nreq, TPB)), dim3(TPB), 0, stream, L.recs, L.shape,
                       L.req_stream, L.start, L.len, (uint32_t)L.nreq, L.content, L.stride, L.tables, L.rstat,
                       L.pathw, L.contra);
    hipLaunchKernelGGL(qread_scan_tile_kernel, tiles, dim3(TPB), 0, stream, L.tables.parents, L.pitch, n, L.sums);
    hipLaunchKernelGGL(qread_scan_sums_kernel, dim3(SCAN_ARRAYS), dim3(TPB), 0, stream, L.sums, L.scan_blocks);
    hipLaunchKernelGGL(qread_scan_add_kernel, tiles, dim3(TPB), 0, stream, L.tables.parents, L.pitch, n, L.sums);
    return hipGetLastError();
}

}  // namespace chip
