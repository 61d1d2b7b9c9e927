// ecies_kernels.hip — KE: AES-256-GCM over a ragged batch of device-resident
// messages.  The arithmetic and the way a message is split are in
// gcm_device.hpp (shared with the host check); this file maps waves to
// messages and items, reduces over the lanes and stores the results.
//
// No address and no branch here depends on a secret: a wave's message and
// item come from blockIdx and the uploaded table, the round keys are read by
// round index through a wave-uniform pointer, the key schedule sits in LDS at
// fixed addresses, and lanes exchange GHASH shares by cross-lane XOR only.
#include "ecies_kernels.hpp"

#include "carbonado_hip.h"

namespace chip {
namespace {

using namespace gcm;

__device__ inline B128 wave_xor(B128 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v.w[j] ^= uint32_t(__shfl_xor(int(v.w[j]), d, 64));
    }
    return v;
}

__global__ __launch_bounds__(64) void gcm_setup_kernel(const uint8_t *__restrict__ raw, KeyMat *__restrict__ km) {
    __shared__ uint32_t kiv[12];
    __shared__ uint32_t w[60];
    __shared__ uint32_t rk[RK_WORDS];
    const uint32_t o = blockIdx.x, lane = threadIdx.x;
    if (lane < 12) kiv[lane] = reinterpret_cast<const uint32_t *>(raw + 48ull * o)[lane];
    __syncthreads();
    if (lane == 0) aes256_expand(reinterpret_cast<const uint8_t *>(kiv), w, rk);
    __syncthreads();
    setup_lane(rk, reinterpret_cast<const uint8_t *>(kiv + 8), lane, &km[o]);
    for (uint32_t i = lane; i < RK_WORDS; i += LANES) km[o].rk[i] = rk[i];
}

template <uint32_t MODE>
__global__ __launch_bounds__(256) void gcm_span_kernel(GcmLaunch L) {
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63;
    if (item >= L.items) return;
    // the last message whose first item is not behind this one (empty messages share a neighbour's)
    uint32_t lo = 0, hi = L.count - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (L.msgs[mid].item0 <= item) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t o = __builtin_amdgcn_readfirstlane(lo);
    const Msg m = L.msgs[o];
    const bool ok = MODE == MODE_CTR ? L.ok[o] != 0 : true;
    B128 v = span_lane<MODE>(&L.km[o], m, item - m.item0, lane, L.in + m.in_off, L.out + m.out_off, ok);
    if (MODE == MODE_CTR) return;
    v = wave_xor(v);
    if (lane == 0) L.vals[item] = v;
}

template <bool SEAL>
__global__ __launch_bounds__(64) void gcm_finish_kernel(GcmLaunch L) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x;
    const Msg m = L.msgs[o];
    const B128 st = wave_xor(finish_lane(&L.km[o], L.vals + m.item0, m.nitems, lane));
    if (lane != 0) return;
    uint32_t t[4];
    final_tag(&L.km[o], st, m.len, t);
    if (SEAL) {
        store_block(L.tag + m.tag_off, t, 16);
    } else {
        uint32_t g[4] = {0, 0, 0, 0};
        if (!m.refused) load_block(L.tag + m.tag_off, 16, g);  // (a refused envelope may be too short to hold one)
        const uint32_t diff = (g[0] ^ t[0]) | (g[1] ^ t[1]) | (g[2] ^ t[2]) | (g[3] ^ t[3]);  // all 16 bytes, no early exit
        const bool good = diff == 0 && !m.refused;
        if (L.keep_status && L.status[o] != 0) {  // failed an earlier stage: not opened, its status stays
            L.ok[o] = 0;
        } else {
            L.ok[o] = good;
            L.status[o] = good ? 0u : uint32_t(CHIP_ERR_ECIES);
        }
    }
}

// The 81 header bytes (eph_pub65 || nonce16) of every envelope, in front of its
// tag: from the scratch slots into the envelopes (seal) or back (open).
template <bool SCATTER>
__global__ __launch_bounds__(256) void gcm_hdr_kernel(const Msg *__restrict__ msgs, uint8_t *hdrs, uint8_t *env,
                                                      uint32_t count) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    const uint32_t o = uint32_t(i / 96), b = uint32_t(i % 96);
    if (o >= count || b >= 81 || msgs[o].refused) return;
    uint8_t *e = env + msgs[o].tag_off - 81 + b;
    if (SCATTER) *e = hdrs[96ull * o + b];
    else hdrs[96ull * o + b] = *e;
}

}  // namespace

hipError_t gcm_hdr_launch(const GcmLaunch &L, uint8_t *hdrs, bool scatter, hipStream_t stream) {
    const dim3 grid(unsigned((uint64_t(L.count) * 96 + 255) / 256)), block(256);
    if (scatter) hipLaunchKernelGGL(gcm_hdr_kernel<true>, grid, block, 0, stream, L.msgs, hdrs, L.tag, L.count);
    else hipLaunchKernelGGL(gcm_hdr_kernel<false>, grid, block, 0, stream, L.msgs, hdrs, L.tag, L.count);
    return hipGetLastError();
}

hipError_t gcm_setup_launch(const GcmLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(gcm_setup_kernel, dim3(L.count), dim3(64), 0, stream, L.rawkeys, L.km);
    return hipGetLastError();
}

hipError_t gcm_span_launch(const GcmLaunch &L, uint32_t mode, hipStream_t stream) {
    if (L.items == 0) return hipSuccess;
    const dim3 grid((L.items + 3) / 4), block(256);
    if (mode == gcm::MODE_SEAL) hipLaunchKernelGGL(gcm_span_kernel<gcm::MODE_SEAL>, grid, block, 0, stream, L);
    else if (mode == gcm::MODE_HASH) hipLaunchKernelGGL(gcm_span_kernel<gcm::MODE_HASH>, grid, block, 0, stream, L);
    else hipLaunchKernelGGL(gcm_span_kernel<gcm::MODE_CTR>, grid, block, 0, stream, L);
    return hipGetLastError();
}

hipError_t gcm_finish_launch(const GcmLaunch &L, bool seal, hipStream_t stream) {
    if (seal) hipLaunchKernelGGL(gcm_finish_kernel<true>, dim3(L.count), dim3(64), 0, stream, L);
    else hipLaunchKernelGGL(gcm_finish_kernel<false>, dim3(L.count), dim3(64), 0, stream, L);
    return hipGetLastError();
}

}  // namespace chip
