// gread_kernels.hip — KG: plaintext ranged reads of level-14 and level-15
// objects planned on the device (gfx950), the kernels behind
// include/carbonado_hip_gread.h that KQ, KA, KD, KV, KC and KK do not already
// supply.
//
//  * gread_rewrite_kernel: one lane per request.  The lane runs gread::decide
//    (gread_device.hpp: refused, killed by the index, or read) and writes the
//    frame-stream request the inner planned read gets in the plaintext
//    request's place: the same stream, off[f0], off[f1 + 1] - off[f0]; a stream
//    index the planner refuses for a refused request, an empty len for a
//    killed or empty one.  20 bytes of stores per lane;
//  * gread_block_kernel: one 64-lane workgroup per (request, k < fcap), the grid
//    a bound from the call's capacity: workgroup w is request w % nreq and frame
//    f0 + w / nreq.  It leaves at once where the request's status word is not 0
//    or the frame is past the request's last; else it builds its fread::Seg in
//    registers from the request and the frame table (no item table, no search)
//    and calls fread::frame_block (fread_block.hpp), the one block decode KF's
//    fread_block_kernel calls too: header against the index,
//    snap::decode_block into 64 KiB of LDS, wave_crc, lane_store of the wanted
//    bytes; then its verdict word;
//  * gread_finish_kernel: one workgroup per request.  It decides the request,
//    leaves where it was refused, stores the content length of every other
//    request and calls fread::finish_request (fread_block.hpp), the one finish
//    KF's fread_finish_kernel feeds from its table: the verdict words combined,
//    zeros and status 16, the read's status or the kill status where needed.
//
// No address and no branch here depends on a secret: requests, frame records,
// entries, status and key_status words are public, and the staged bytes a
// block decode is driven by are the object's data, as in KF.  No store leaves
// the request's scratch words, its slot's [0, content length) or its result
// words.
#include "gread_kernels.hpp"

#include "fread_block.hpp"

namespace chip {
namespace {

using namespace gread;

__device__ inline Decision decide_request(const GreadLaunch &L, uint32_t r) {
    return decide(L.recs, L.frecs, L.ent, L.key_status, L.shape, L.req_stream[r], L.start[r], L.len[r]);
}

__global__ __launch_bounds__(256) void gread_rewrite_kernel(GreadLaunch L) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= L.nreq) return;
    const Decision d = decide_request(L, r);
    L.q_stream[r] = d.q_stream;
    L.q_start[r] = d.q_start;
    L.q_len[r] = d.q_len;
}

__global__ __launch_bounds__(64) void gread_block_kernel(GreadLaunch L) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[FRAME];
    __shared__ uint32_t tab[256];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    // k-major: the first nreq workgroups are every request's first frame.  Request-major, a 4 KiB read's
    // grid alternates a decoding workgroup with one that leaves at once, and the kernel took twice as long
    // (supposedly consecutive workgroups go round the 8 XCDs and every other XCD got no decode)
    const uint32_t r = w % L.nreq, k = w / L.nreq;
    // the read failed, or the request was refused or killed by its key: the finish kernel zeroes what there is
    // to zero.  Its bad word stays unwritten: gread_finish_kernel looks at a request's bad words only where its status
    // word is still 0, and then every one of its frames' words was written
    if (L.status[r] != 0) return;
    const Decision d = decide_request(L, r);
    if (d.order != READ || k >= d.nfr) return;
    const fread::Seg sg = item_of_request(L.frecs[d.q_stream], L.ent, d, r, k, L.stage_stride, L.stride);
    const bool ok = fread::frame_block(sg, L.stage, L.content, stage, tab, lane);
    if (lane == 0) L.bad[(uint64_t)r * L.shape.fcap + k] = ok ? 0u : 1u;
}

__global__ __launch_bounds__(256) void gread_finish_kernel(GreadLaunch L) {
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const Decision d = decide_request(L, r);
    if (d.order == REFUSED) {  // the inner planner wrote its words
        if (tid == 0) L.content_len[r] = 0;
        return;
    }
    if (tid == 0) L.content_len[r] = d.n;
    const uint32_t kill = d.order == KILLED ? d.kill : L.key_status ? L.key_status[d.q_stream] : 0u;
    fread::finish_request(kill, d.n, L.bad + (uint64_t)r * L.shape.fcap, d.nfr, L.content + (uint64_t)r * L.stride,
                          L.status, L.used, L.vouch, r, tid);
}

}  // namespace

hipError_t gread_rewrite_launch(const GreadLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(gread_rewrite_kernel, dim3((L.nreq + 255) / 256), dim3(256), 0, stream, L);
    return hipGetLastError();
}

hipError_t gread_block_launch(const GreadLaunch &L, hipStream_t stream) {
    const uint64_t work = (uint64_t)L.nreq * L.shape.fcap;  // below 2^31 (gread::Geometry)
    hipLaunchKernelGGL(gread_block_kernel, dim3((unsigned)work), dim3(fread::LANES), 0, stream, L);
    return hipGetLastError();
}

hipError_t gread_finish_launch(const GreadLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(gread_finish_kernel, dim3(L.nreq), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace chip
