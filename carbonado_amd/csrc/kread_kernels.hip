// kread_kernels.hip — KK: plaintext ranged reads of level-13 objects planned
// on the device (gfx950), the kernels behind include/carbonado_hip_kread.h
// that KQ, KA, KD, KV and KC do not already supply.
//
//  * kread_rewrite_kernel: one lane per request.  The lane runs kread::decide
//    (kread_device.hpp: refused, killed, or read) and writes the envelope
//    request KQ's planner gets in the plaintext request's place: the same
//    stream, start + 97, the same len; a stream index the planner refuses for
//    a refused request, an empty len for a killed one.  20 bytes of stores per
//    lane;
//  * kread_ctr_kernel: one wave per (request, span of 127 units), the grid a
//    bound from the call's capacity: wave w is request w / cap, span w % cap.
//    The wave builds its cread::Item in registers from the request (no item
//    table, no search), takes its key from the resident key table by the
//    request's stream index through a wave-uniform pointer and runs the lane
//    functions of cread_device.hpp exactly as KC's ctr_range_kernel does,
//    the neighbour's block through a lane shuffle.  A wave past its request's
//    content, or whose request's status word is not 0, leaves at once.  The
//    waves of a killed request store its zeros, span 0 its result words
//    (cread::lane_kill, as KC) and its content length;
//  * kread_table_finish_kernel, behind KC's ctr_setup_kernel when a key table
//    is made: zeros over the raw key records, and over the record of every
//    stream whose key_status is not 0.
//
// No address and no branch here depends on a secret: a wave's request, span
// and key index come from blockIdx and public words (stream indices, lengths,
// status and key_status words); round keys are read by round index.
#include "kread_kernels.hpp"

namespace chip {
namespace {

using namespace kread;

__global__ __launch_bounds__(256) void kread_rewrite_kernel(KreadLaunch L) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= L.nreq) return;
    const Decision d = decide(L.recs, L.key_status, L.shape, L.req_stream[r], L.start[r], L.len[r]);
    L.q_stream[r] = d.q_stream;
    L.q_start[r] = d.q_start;
    L.q_len[r] = d.q_len;
}

__global__ __launch_bounds__(256) void kread_ctr_kernel(KreadLaunch L) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = w / L.cap, span = w % L.cap;
    if (r >= L.nreq) return;
    const uint32_t s = __builtin_amdgcn_readfirstlane(L.q_stream[r]);
    if (s >= L.shape.nstreams) return;  // refused by the rewrite: the planner wrote its words
    const uint32_t kill = __builtin_amdgcn_readfirstlane(L.key_status[s]);
    uint8_t *buf = L.content + (uint64_t)r * L.stride;
    if (kill) {  // no keystream, no gate; the length is the decision's, the planner saw an empty request
        const Decision d = decide(L.recs, L.key_status, L.shape, L.req_stream[r], L.start[r], L.len[r]);
        const cread::Item it = item_of_request(r, L.stride, L.start[r], d.clen, s, kill);
        if (span >= cread::work_of(it.n, kill)) return;
        if (span == 0 && lane == 0) L.content_len[r] = it.n;
        cread::lane_kill(it, span, lane, buf, L.status, L.used, L.vouch, r);
        return;
    }
    const cread::Item it = item_of_request(r, L.stride, L.start[r], L.content_len[r], s, 0);
    if (span >= cread::spans_of(it.n)) return;
    if (__builtin_amdgcn_readfirstlane(L.status[r]) != 0) return;
    uint32_t ka[4] = {0, 0, 0, 0}, kb[4] = {0, 0, 0, 0}, kn[4];
    if (cread::lane_needed(it, span, lane)) cread::lane_eval(&L.km[s], it, span, lane, ka, kb);
#pragma unroll
    for (int c = 0; c < 4; ++c) kn[c] = uint32_t(__shfl_down(int(ka[c]), 1, 64));
    cread::lane_apply(it, span, lane, ka, kb, kn, buf);
}

__global__ __launch_bounds__(256) void kread_table_finish_kernel(cread::CtrKey *km, const uint32_t *key_status,
                                                                 uint8_t *raw, uint32_t nstreams) {
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= nstreams) return;
    if (lane < cread::RAW_KEY / 4) reinterpret_cast<uint32_t *>(raw + cread::RAW_KEY * s)[lane] = 0;
    uint32_t *rec = reinterpret_cast<uint32_t *>(km + s);
    if (key_status[s] != 0) {
        for (uint32_t i = lane; i < sizeof(cread::CtrKey) / 4; i += 64) rec[i] = 0;
    } else if (lane < 4) {
        km[s].pad_[lane] = 0;  // the setup kernel leaves the padding as it found it
    }
}

}  // namespace

hipError_t kread_rewrite_launch(const KreadLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(kread_rewrite_kernel, dim3((L.nreq + 255) / 256), dim3(256), 0, stream, L);
    return hipGetLastError();
}

hipError_t kread_ctr_launch(const KreadLaunch &L, hipStream_t stream) {
    const uint64_t work = (uint64_t)L.nreq * L.cap;  // below 2^31 (kread::Geometry)
    hipLaunchKernelGGL(kread_ctr_kernel, dim3((unsigned)((work + 3) / 4)), dim3(256), 0, stream, L);
    return hipGetLastError();
}

hipError_t kread_table_finish_launch(cread::CtrKey *km, const uint32_t *key_status, uint8_t *raw, uint32_t nstreams,
                                     hipStream_t stream) {
    hipLaunchKernelGGL(kread_table_finish_kernel, dim3((unsigned)(((uint64_t)nstreams + 3) / 4)), dim3(256), 0, stream,
                       km, key_status, raw, nstreams);
    return hipGetLastError();
}

}  // namespace chip
