// cread_kernels.hip — KC: AES-256-GCM's keystream XORed over byte ranges of
// device memory in place, for plaintext ranged reads of encrypted objects.
// The arithmetic and the way an item is split are in cread_device.hpp (shared
// with the host check); this file maps waves to keys and work items and moves
// one keystream block between neighbouring lanes.
//
// No address and no branch here depends on a secret: a wave's key, item and
// span come from blockIdx and the uploaded table, the round keys are read by
// round index through a wave-uniform pointer, the key schedule sits in LDS at
// fixed addresses, and the neighbour's block travels through a lane shuffle
// (registers only).
#include "cread_kernels.hpp"

namespace chip {
namespace {

using namespace cread;

__global__ __launch_bounds__(64) void ctr_setup_kernel(const uint8_t *__restrict__ raw, CtrKey *__restrict__ km) {
    __shared__ uint32_t kiv[12];
    __shared__ uint32_t w[60];
    __shared__ uint32_t rk[gcm::RK_WORDS];
    __shared__ uint32_t j0[4];
    const uint32_t o = blockIdx.x, lane = threadIdx.x;
    if (lane < 12) kiv[lane] = reinterpret_cast<const uint32_t *>(raw + RAW_KEY * o)[lane];
    __syncthreads();
    if (lane == 0) {
        gcm::aes256_expand(reinterpret_cast<const uint8_t *>(kiv), w, rk);
        setup_lite(rk, reinterpret_cast<const uint8_t *>(kiv + 8), j0);
    }
    __syncthreads();
    for (uint32_t i = lane; i < gcm::RK_WORDS; i += LANES) km[o].rk[i] = rk[i];
    if (lane < 4) km[o].j0[lane] = j0[lane];
}

__global__ __launch_bounds__(256) void ctr_range_kernel(CtrLaunch L) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63;
    if (w >= L.work) return;
    const uint32_t i = __builtin_amdgcn_readfirstlane(item_of(L.items, L.nitems, w));
    const Item it = L.items[i];
    const uint32_t span = w - it.work0;
    uint8_t *buf = L.buf + it.buf_off;
    if (it.kill) {  // decided on the host: no keystream, no gate
        lane_kill(it, span, lane, buf, L.status, L.used, L.vouch, i);
        return;
    }
    if (L.gate && __builtin_amdgcn_readfirstlane(L.gate[i]) != 0) return;
    uint32_t ka[4] = {0, 0, 0, 0}, kb[4] = {0, 0, 0, 0}, kn[4];
    if (lane_needed(it, span, lane)) lane_eval(&L.km[it.key], it, span, lane, ka, kb);
#pragma unroll
    for (int c = 0; c < 4; ++c) kn[c] = uint32_t(__shfl_down(int(ka[c]), 1, 64));
    lane_apply(it, span, lane, ka, kb, kn, buf);
}

}  // namespace

hipError_t ctr_setup_launch(const CtrLaunch &L, hipStream_t stream) {
    if (L.keys_used == 0) return hipSuccess;
    hipLaunchKernelGGL(ctr_setup_kernel, dim3(L.keys_used), dim3(64), 0, stream, L.rawkeys, L.km);
    return hipGetLastError();
}

hipError_t ctr_range_launch(const CtrLaunch &L, hipStream_t stream) {
    if (L.work == 0) return hipSuccess;
    hipLaunchKernelGGL(ctr_range_kernel, dim3((L.work + 3) / 4), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace chip
