// mul_probe.hip — gfx950 rate of the 32 x 32 -> 64-bit multiply-add
// (v_mad_u64_u32, the one multiply the secp256k1 field of
// carbonado_amd/csrc/agree_device.hpp compiles to) and of agree::fe_mul itself.
// Calibration tool beside valu_probe.hip: it settles the figure DESIGN.md
// prices the key agreement kernels against.
//
// mad:    every lane runs C chains of v_mad_u64_u32 (inline asm, so nothing is
//         folded), C = 1 for the dependent latency and C = 8 for the issue rate;
// fe_mul: every lane runs a chain of field multiplications a = a b, as the
//         inversion and the point formulas do.
// Grid = 1024 W blocks of one wave, W waves per SIMD on 256 CUs when every
// block is resident.  Every wave stamps clock64() around its loop: the report
// carries cycles per instruction (per fe_mul) per wave beside the wall clock.
//
//   hipcc -O3 --offload-arch=gfx950 -I carbonado_amd/csrc tools/mul_probe.hip -o tools/mul_probe
//   tools/mul_probe [iters=20000]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "agree_device.hpp"

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e = (x);                                                          \
        if (e != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

template <int C>
__global__ __launch_bounds__(64) void mad_kernel(uint64_t *out, uint64_t *cycles, uint32_t iters) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    uint64_t acc[C];
    for (int c = 0; c < C; ++c) acc[c] = t * 0x9E3779B97F4A7C15ull + c;
    const uint32_t a = t | 1u, b = (t << 7) | 3u;
    const uint64_t t0 = clock64();
    for (uint32_t i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < C; ++c) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[c]) : "v"(a), "v"(b) : "vcc");
    }
    const uint64_t t1 = clock64();
    uint64_t x = 0;
    for (int c = 0; c < C; ++c) x ^= acc[c];
    out[t] = x;
    if (threadIdx.x == 0) cycles[blockIdx.x] = t1 - t0;
}

__global__ __launch_bounds__(64) void fe_kernel(uint32_t *io, uint64_t *cycles, uint32_t iters) {
    using namespace chip::agree;
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    Fe a, b;
    for (int i = 0; i < 8; ++i) a.v[i] = io[i] ^ t, b.v[i] = io[8 + i] + t;
    const uint64_t t0 = clock64();
#pragma unroll 1
    for (uint32_t i = 0; i < iters; ++i) a = fe_mul(a, b);
    const uint64_t t1 = clock64();
    uint32_t x = 0;
    for (int i = 0; i < 8; ++i) x ^= a.v[i];
    io[16 + t] = x;
    if (threadIdx.x == 0) cycles[blockIdx.x] = t1 - t0;
}

static double median_cycles(const uint64_t *d, size_t n) {
    std::vector<uint64_t> h(n);
    CK(hipMemcpy(h.data(), d, n * 8, hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    return double(h[n / 2]);
}

int main(int argc, char **argv) {
    const uint32_t iters = argc > 1 ? uint32_t(atoi(argv[1])) : 20000;
    const int maxw = 4, blocks1 = 1024;
    uint64_t *out, *cycles;
    uint32_t *io;
    CK(hipMalloc(&out, size_t(blocks1) * maxw * 64 * 8));
    CK(hipMalloc(&cycles, size_t(blocks1) * maxw * 8));
    CK(hipMalloc(&io, (16 + size_t(blocks1) * maxw * 64) * 4));
    CK(hipMemset(io, 0x5A, 64));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    printf("{\"tool\": \"mul_probe\", \"iters\": %u, \"rows\": [", iters);
    bool first = true;
    for (int kind = 0; kind < 3; ++kind) {
        for (int w = 1; w <= maxw; w *= 2) {
            const int blocks = blocks1 * w;
            const int per_iter = kind == 1 ? 8 : 1;
            for (int rep = 0; rep < 2; ++rep) {  // the first is the warm-up
                CK(hipEventRecord(e0));
                if (kind == 0) hipLaunchKernelGGL(mad_kernel<1>, dim3(blocks), dim3(64), 0, 0, out, cycles, iters);
                if (kind == 1) hipLaunchKernelGGL(mad_kernel<8>, dim3(blocks), dim3(64), 0, 0, out, cycles, iters);
                if (kind == 2) hipLaunchKernelGGL(fe_kernel, dim3(blocks), dim3(64), 0, 0, io, cycles, iters / 16);
                CK(hipGetLastError());
                CK(hipEventRecord(e1));
                CK(hipEventSynchronize(e1));
            }
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            const double n = kind == 2 ? double(iters / 16) : double(iters) * per_iter;
            printf("%s{\"what\": \"%s\", \"waves_per_simd\": %d, \"cycles_per_op_per_wave\": %.2f, \"ms\": %.3f}",
                   first ? "" : ", ", kind == 0 ? "v_mad_u64_u32 dependent" : kind == 1 ? "v_mad_u64_u32 x8" : "fe_mul chain",
                   w, median_cycles(cycles, blocks) / n, ms);
            first = false;
        }
    }
    printf("]}\n");
    return 0;
}
