// snap_wave.hpp — what one wave does together for snap_device.hpp's block
// coder, and the CRC-32C of a block by one wave: shared by KZ
// (snap_kernels.hip) and KF (fread_kernels.hip).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "snap_device.hpp"

namespace chip {
namespace snap {

// What a wave does together (snap_device.hpp).  Control flow around these is
// wave-uniform: every lane reads the same tag and table bytes.
struct Wave {
    uint32_t lane;
    __device__ void copy(uint8_t *dst, const uint8_t *src, size_t n) const {
        for (size_t i = lane; i < n; i += LANES) dst[i] = src[i];
    }
    __device__ size_t match(const uint8_t *src, size_t a, size_t b, size_t n) const {
        for (size_t base = 0;; base += 8 * LANES) {
            const size_t at = base + 8 * lane;
            uint32_t c = 0;
            bool go = true;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const bool in = b + at + k < n;
                const uint8_t x = in ? src[a + at + k] : uint8_t(0);
                const uint8_t y = in ? src[b + at + k] : uint8_t(1);
                go = go && x == y;
                c += go ? 1u : 0u;
            }
            const unsigned long long stop = __ballot(c < 8);
            if (stop) {  // (a lane at or past the block's end always stops)
                const int first = __builtin_ctzll(stop);
                return base + 8 * size_t(first) + size_t(__shfl(int(c), first, LANES));
            }
        }
    }
    __device__ void zero16(uint16_t *t, size_t n) const {
        uint32_t *t32 = reinterpret_cast<uint32_t *>(t);
        for (size_t i = lane; i < n / 2; i += LANES) t32[i] = 0;
    }
    __device__ void put(uint8_t *p, uint8_t v) const {
        if (lane == 0) *p = v;
    }
    __device__ void rep(uint8_t *stage, size_t d, size_t off, size_t c) const {
        const uint32_t i = off >= LANES ? lane : lane % uint32_t(off);
        uint8_t v = 0;
        if (lane < c) v = stage[d - off + i];
        if (lane < c) stage[d + lane] = v;
    }
    __device__ void sync() const { __syncthreads(); }
    __device__ uint32_t uni(uint32_t x) const { return __builtin_amdgcn_readfirstlane(x); }
};

__device__ inline uint32_t wave_xor32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= uint32_t(__shfl_xor(int(v), d, LANES));
    return v;
}

// 256 entries by the block's first 64 threads; the caller synchronises
__device__ inline void crc_table_fill(uint32_t *tab, uint32_t lane) {
    for (uint32_t i = lane; i < 256; i += LANES) tab[i] = crc_table_entry(i);
}

// masked CRC-32C of p[0, n) by one wave (every lane returns it)
__device__ inline uint32_t wave_crc(const uint32_t *tab, const uint8_t *p, size_t n, uint32_t lane) {
    return crc_finish(wave_xor32(crc_lane_term(tab, p, n, lane)), n);
}

}  // namespace snap
}  // namespace chip
