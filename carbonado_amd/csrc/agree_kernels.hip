// agree_kernels.hip — KY: the Ecies key agreement over a batch.  The
// arithmetic and the way a multiplication is split over lanes are in
// agree_device.hpp (shared with the host check); this file maps waves and
// lanes to objects, exchanges points between lanes and stores the results.
//
// No address and no branch here depends on a secret: an object comes from
// blockIdx / threadIdx, a lane's window is cut from the one scalar word its
// lane index names, tables are scanned whole under masks, lanes exchange
// points by cross-lane moves only, and the one branch of the open kernel is
// on the parse of a PUBLIC ephemeral key.  Both kernels keep every secret in
// registers (private segment 0 bytes, no LDS).
#include "agree_kernels.hpp"

#include "qread_device.hpp"

namespace chip {
namespace {

using namespace agree;

__device__ inline Fe fe_from_lane(const Fe &a, uint32_t m) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = uint32_t(__shfl_xor(int(a.v[i]), int(m), 64));
    return r;
}

__device__ inline void store_bytes32(uint8_t *dst, const Sha &s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        dst[4 * i] = uint8_t(s.h[i] >> 24), dst[4 * i + 1] = uint8_t(s.h[i] >> 16);
        dst[4 * i + 2] = uint8_t(s.h[i] >> 8), dst[4 * i + 3] = uint8_t(s.h[i]);
    }
}

__global__ __launch_bounds__(64) void agree_seal_kernel(AgreeSeal L) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x;
    const uint32_t w = window_of(L.sk[8ull * o + (lane >> 3)], lane);
    Pt e = pt_inf(), s = pt_inf();
#pragma unroll 1
    for (int b = 0; b < 2; ++b) {  // k G, then k P: one copy of the addition
        Pt p = comb_pick(b ? L.ptab : L.gtab, lane, w);
#pragma unroll 1
        for (uint32_t m = 1; m < LANES; m <<= 1) {
            const Pt q{fe_from_lane(p.x, m), fe_from_lane(p.y, m), fe_from_lane(p.z, m)};
            p = pt_add(p, q);
        }
        if (b == 0) e = p;
        else s = p;
    }
    Fe ex, ey, sx, sy;
    affine_pair(e, s, ex, ey, sx, sy);
    const Sha key = hkdf_points(0x04, ex, ey, sx, sy);
    if (lane != 0) return;
    uint8_t *pub = L.pub + o * L.pub_pitch;
    pub[0] = 0x04;
    fe_to_be(ex, pub + 1);
    fe_to_be(ey, pub + 33);
    store_bytes32(L.keys + o * L.key_pitch, key);
}

__global__ __launch_bounds__(64) void agree_open_kernel(AgreeOpen L) {
    const uint32_t o = blockIdx.x * LANES + threadIdx.x;
    if (o >= L.count) return;
    const uint8_t *eph = L.eph + o * L.eph_pitch;
    uint8_t *key = L.keys + o * L.key_pitch;
    Fe x, y;
    uint32_t st = L.gate ? L.gate[o] : 0u;
    if (L.shorter && L.shorter[o]) st = ERR_ECIES;
    if (!st) st = parse65(eph, x, y);
    if (L.status) L.status[o] = st;
    if (L.copy_iv) {
#pragma unroll
        for (int i = 0; i < 16; ++i) key[32 + i] = st ? uint8_t(0) : eph[65 + i];
    }
    if (st) {  // public: the header could not be read, the object is no envelope or its ephemeral key does not parse
        if (L.refused) *reinterpret_cast<uint32_t *>(L.refused + o * L.refused_stride) = 1;
#pragma unroll
        for (int i = 0; i < 32; ++i) key[i] = 0;
        return;
    }
    var_table(L.vtab, o, x, y);
    Fe sx, sy;
    affine(var_mul(L.vtab, o, L.sk), sx, sy);
    store_bytes32(key, hkdf_points(eph[0], x, y, sx, sy));
}

__global__ __launch_bounds__(256) void agree_requests_kernel(AgreeRequests L) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= L.nstreams) return;
    const qread::StreamRec r = static_cast<const qread::StreamRec *>(L.recs)[s];
    const uint32_t shorter = r.C != 0 && 4ull * r.C - r.padding < 97;
    L.req_stream[s] = s;
    L.start[s] = 0;
    L.len[s] = shorter ? 0 : 81;
    L.shorter[s] = shorter;
}

}  // namespace

hipError_t agree_requests_launch(const AgreeRequests &L, hipStream_t stream) {
    hipLaunchKernelGGL(agree_requests_kernel, dim3((L.nstreams + 255) / 256), dim3(256), 0, stream, L);
    return hipGetLastError();
}

hipError_t agree_seal_launch(const AgreeSeal &L, hipStream_t stream) {
    hipLaunchKernelGGL(agree_seal_kernel, dim3(L.count), dim3(LANES), 0, stream, L);
    return hipGetLastError();
}

hipError_t agree_open_launch(const AgreeOpen &L, hipStream_t stream) {
    hipLaunchKernelGGL(agree_open_kernel, dim3((L.count + LANES - 1) / LANES), dim3(LANES), 0, stream, L);
    return hipGetLastError();
}

}  // namespace chip
