// repair_kernels.hip — KP: the repair half of the ragged scrub (gfx950), the
// kernels behind include/carbonado_hip_repair.h that KR and KA do not already
// supply.
//
// A pass is a table of streams to repair (repair_plan.hpp: repair::Rec /
// repair::Commit) with prefix arrays of work per repair, so every launch
// covers all repairs of the pass whatever their lengths and share patterns:
//
//  * repair_decode_kernel: rag_parity_kernel<1> run backwards.  A workgroup
//    finds its (repair, 4 KiB block) by binary search on blockIdx.x; each lane
//    reads 16 B at the same position of the 4 selected shares straight from
//    their chunk slots of the damaged stream (chunk_stream_off, 8-B aligned
//    loads: no gather of the content first), multiplies by the repair's own
//    4 x 4 inverse through a packed product table in LDS (parity16's layout:
//    entry [s][x] = byte r holds coef[r][s] * x, then a 4 x 4 byte transpose)
//    and writes 16 B of each of the 4 primaries, contiguous and 16-B aligned.
//    The table is built by the workgroup from the record's 16 coefficients:
//    lane x carries the four packed coefficient words through the 8 doublings
//    of GF(2^8) (0x11D) and accumulates those of x's set bits, ~100 VALU per
//    lane against 4 loads + 16 table products per 16 B, so any mix of share
//    patterns shares one launch and nothing is uploaded per pattern.  A
//    selected share that is a primary has a unit row: multiplication by 1,
//    the same path;
//  * repair_fold_kernel: 8 request status words of KA's verify into a mask;
//  * repair_compare_kernel / repair_commit_kernel: the re-encoded hash against
//    the expected one, then the rows that matched to their output ranges,
//    16 B per lane; a row that did not match is not read.
#include "bao_device.hpp"
#include "chip_internal.hpp"
#include "repair_kernels.hpp"
#include "zfec_device.hpp"

namespace chip {

using namespace bao;

namespace repair {

constexpr int TPB = 256;
static_assert(BLOCK == 16 * TPB, "bytes of a share per workgroup");

// 16 B of the four output rows from 16 B at the same position of each input
// (ragged_kernels.hip parity16: the packed table in LDS, a 4 x 4 transpose)
__device__ __forceinline__ void product16(const uint32_t *tab, const u32x4 (&v)[4], u32x4 (&p)[4]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        uint32_t acc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            uint32_t x = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) x ^= tab[j * 256 + ((zf::comp(v[j], d) >> (8 * b)) & 0xFFu)];
            acc[b] = x;
        }
        uint32_t r0, r1, r2, r3;
        zf::transpose4(acc[0], acc[1], acc[2], acc[3], r0, r1, r2, r3);
        if (d == 0) { p[0].x = r0; p[1].x = r1; p[2].x = r2; p[3].x = r3; }
        if (d == 1) { p[0].y = r0; p[1].y = r1; p[2].y = r2; p[3].y = r3; }
        if (d == 2) { p[0].z = r0; p[1].z = r1; p[2].z = r2; p[3].z = r3; }
        if (d == 3) { p[0].w = r0; p[1].w = r1; p[2].w = r2; p[3].w = r3; }
    }
}

__global__ __launch_bounds__(TPB) void repair_decode_kernel(const Rec *recs, const uint32_t *blocks, uint32_t nrep) {
    __shared__ uint32_t tab[4 * 256];
    const uint32_t rep = audit::prefix_find<uint32_t>(blocks, nrep, blockIdx.x);
    const Rec a = recs[rep];
    const uint32_t x = threadIdx.x;
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // tab[s][x]: byte r = coef[4 r + s] * x
        uint32_t cw = (uint32_t)a.coef[s] | (uint32_t)a.coef[4 + s] << 8 | (uint32_t)a.coef[8 + s] << 16 |
                      (uint32_t)a.coef[12 + s] << 24;
        uint32_t acc = 0;
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            if (x >> bit & 1) acc ^= cw;
            cw = zf::gf_double4(cw);
        }
        tab[s * 256 + x] = acc;
    }
    const uint64_t C = a.C, o = 16 * ((uint64_t)(blockIdx.x - blocks[rep]) * TPB + threadIdx.x);
    const uint64_t cols = C / 1024, u = o / 1024, w = o % 1024;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    u32x4 v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
        v[s] = o < C ? load16_a8(src + chunk_stream_off(a.sel[s] * cols + u, a.N) + w) : u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    if (o >= C) return;
    u32x4 p[4];
    product16(tab, v, p);
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.dst);
#pragma unroll
    for (int r = 0; r < 4; ++r) *glb(reinterpret_cast<u32x4 *>(dst + r * C + o)) = p[r];
}

__global__ __launch_bounds__(TPB) void repair_fold_kernel(const uint32_t *rstat, const uint32_t *first, uint32_t count,
                                                          uint32_t *masks) {
    const uint32_t o = blockIdx.x * TPB + threadIdx.x;
    if (o >= count) return;
    const uint32_t r0 = first[o], nr = first[o + 1] - r0;
    uint32_t m = 0;
    for (uint32_t i = 0; i < nr; ++i) m |= (rstat[r0 + i] == 0 ? 1u : 0u) << i;
    masks[o] = m;
}

__global__ __launch_bounds__(TPB) void repair_compare_kernel(const Commit *commits, uint32_t nrep, uint32_t *ok) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= nrep) return;
    const uint8_t *want = reinterpret_cast<const uint8_t *>(commits[j].want);  // any alignment
    const uint8_t *got = reinterpret_cast<const uint8_t *>(commits[j].got);
    uint32_t diff = 0;
    for (int i = 0; i < 32; ++i) diff |= (uint32_t)(want[i] ^ got[i]);
    ok[j] = diff == 0 ? 1u : 0u;
}

__global__ __launch_bounds__(TPB) void repair_commit_kernel(const Commit *commits, const uint64_t *pre, uint32_t nrep,
                                                            uint64_t total, const uint32_t *ok) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const uint32_t j = audit::prefix_find(pre, nrep, i);
    if (!ok[j]) return;
    const Commit a = commits[j];
    const uint64_t o = UNIT * (i - pre[j]), left = a.len - o;  // a multiple of 8
    const uint8_t *row = reinterpret_cast<const uint8_t *>(a.row) + o;
    uint8_t *out = reinterpret_cast<uint8_t *>(a.out) + o;
    if (left >= 16) store16_a8<false>(out, load16_a8(row));
    else store8<false>(out, *reinterpret_cast<const u32x2 *>(row));
}

}  // namespace repair

hipError_t repair_fold_launch(const uint32_t *rstat, const uint32_t *first, uint32_t count, uint32_t *masks,
                              hipStream_t stream) {
    using namespace repair;
    if (count)
        hipLaunchKernelGGL(repair_fold_kernel, dim3(nblocks(count, TPB)), dim3(TPB), 0, stream, rstat, first, count,
                           masks);
    return hipGetLastError();
}

hipError_t repair_decode_launch(const repair::Rec *recs, const uint32_t *blocks, uint32_t nrep, uint64_t total_blocks,
                                hipStream_t stream) {
    using namespace repair;
    if (total_blocks)
        hipLaunchKernelGGL(repair_decode_kernel, dim3((unsigned)total_blocks), dim3(TPB), 0, stream, recs, blocks, nrep);
    return hipGetLastError();
}

hipError_t repair_commit_launch(const repair::Commit *commits, const uint64_t *units, uint32_t nrep,
                                uint64_t total_units, uint32_t *ok, hipStream_t stream) {
    using namespace repair;
    if (!nrep) return hipSuccess;
    hipLaunchKernelGGL(repair_compare_kernel, dim3(nblocks(nrep, TPB)), dim3(TPB), 0, stream, commits, nrep, ok);
    if (total_units)
        hipLaunchKernelGGL(repair_commit_kernel, dim3(nblocks(total_units, TPB)), dim3(TPB), 0, stream, commits, units,
                           nrep, total_units, ok);
    return hipGetLastError();
}

}  // namespace chip
