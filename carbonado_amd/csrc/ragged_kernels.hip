// ragged_kernels.hip — KR: `count` objects of different lengths per launch
// (gfx950), the kernels behind include/carbonado_hip_ext.h.
//
// The uniform batch kernels (K13, K3, K1) take one n for the whole batch; KM
// (multi_kernels.hip) spreads ONE object over the chip.  KR is KM's work
// driven by a table of objects (ragged_plan.hpp: ragged::Obj) with a prefix
// array of workgroups per object: a workgroup finds its (object, local index)
// by binary search on blockIdx.x, every stream offset is arithmetic
// (chunk_stream_off / parent_stream_off), so a call is a constant number of
// launches whatever the mix of lengths:
//
//  * rag_parity_kernel (Zfec, Zfec|Bao): parity_kernel's work, 4 KiB of every
//    shard per workgroup; the 8 shards shard-major (Zfec) or into the chunk
//    slots of the object's own stream (Zfec|Bao);
//  * rag_group_kernel (Bao, Zfec|Bao; encode / decode): km_kernel's phases 1-3
//    for one aligned group of 64 chunks of one object, a quad of lanes per
//    chunk.  An object of at most 64 chunks has its root inside its only
//    group, which finalizes it (KS's case: N = 1 makes the chunk the root,
//    n = 0 the empty chunk); otherwise the group's CV goes to scratch;
//  * rag_top_kernel: one workgroup per object of more than one group walks
//    levels 7 .. root over its group CVs (km_top's walk).  A launch of its
//    own: the kernel boundary makes the CVs visible, no workgroup waits on
//    another and there is no counter to reset;
//  * rag_copy_kernel (Zfec-only decode): the primaries' bytes out.
//
// Decode never lets one object's damage reach another: a workgroup touches
// one object's bytes and only that object's status word.
#include "bao_device.hpp"
#include "chip_internal.hpp"
#include "quad_b3.hpp"
#include "ragged_kernels.hpp"
#include "zfec_device.hpp"

namespace chip {

using namespace bao;

namespace ragged {

constexpr int TPB = 256, QUADS = TPB / 4;
constexpr int S = (int)GROUP, LOGS = 6;
constexpr int GMAX = (int)TOP_MAX_G;
static_assert(S == QUADS && (1 << LOGS) == S, "one quad per chunk of a group");
static_assert(PARITY_BLOCK == 16 * TPB && COPY_BLOCK == 4 * 16 * TPB, "bytes per workgroup");
static_assert((uint64_t)GMAX * S == KM_MAX_N, "the largest object's stream");

// the object of workgroup b: pre[o] <= b < pre[o + 1] (pre[0] = 0, pre[count] = gridDim.x)
__device__ __forceinline__ uint32_t find_obj(const uint32_t *pre, uint32_t count, uint32_t b) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// 16 B of the four parity shards from 16 B at the same position of each data
// shard (multi_kernels.hip parity16: the packed table in LDS, a 4 x 4 transpose)
__device__ __forceinline__ void parity16(const uint32_t *tab, const u32x4 (&v)[4], u32x4 (&p)[4]) {
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

// BAO 0: shard-major [S0 .. S7] at a.stream (16-B aligned); BAO 1: every
// shard into its chunk slots of the stream at a.stream (8-B aligned).
template <int BAO>
__global__ __launch_bounds__(TPB) void rag_parity_kernel(const Obj *objs, const uint32_t *blocks, uint32_t count,
                                                         const uint32_t *table) {
    __shared__ uint32_t tab[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += TPB) tab[i] = table[i];
    const uint32_t obj = find_obj(blocks, count, blockIdx.x);
    const Obj a = objs[obj];
    const uint64_t C = a.C, o = 16 * ((uint64_t)(blockIdx.x - blocks[obj]) * TPB + threadIdx.x);
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = o < C ? zf::load16_masked(a.src, j * C + o, a.valid) : u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    if (o >= C) return;
    u32x4 p[4];
    parity16(tab, v, p);
    const uint64_t cols = C / 1024, u = o / 1024, w = o % 1024;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const u32x4 x = s < 4 ? v[s] : p[s - 4];
        if (BAO) store16_a8<false>(a.stream + chunk_stream_off(s * cols + u, a.N) + w, x);
        else *glb(reinterpret_cast<u32x4 *>(a.stream + s * C + o)) = x;
    }
}

// Zfec-only decode: bytes [0, out_limit) of the shard buffer (the positional
// primaries) to a.out; both 16-B aligned.
__global__ __launch_bounds__(TPB) void rag_copy_kernel(const Obj *objs, const uint32_t *blocks, uint32_t count) {
    const uint32_t obj = find_obj(blocks, count, blockIdx.x);
    const Obj a = objs[obj];
    const uint64_t base = (uint64_t)(blockIdx.x - blocks[obj]) * COPY_BLOCK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t o = base + 16 * (uint64_t)(i * TPB + threadIdx.x);
        if (o >= a.out_limit) continue;
        const uint64_t left = a.out_limit - o;
        if (left >= 16) *glb(reinterpret_cast<u32x4 *>(a.out + o)) = *reinterpret_cast<const u32x4 *>(a.stream + o);
        else store16_partial(a.out + o, load16_partial(a.stream + o, (uint32_t)left), (uint32_t)left);
    }
}

// the root's CV words of my lane: written (encode) or compared (decode)
template <int MODE>
__device__ __forceinline__ bool root_out(uint8_t *hash, int q, uint32_t h0, uint32_t h1) {
    uint32_t *hp = reinterpret_cast<uint32_t *>(hash);
    if (MODE == 0) {
        hp[q] = h0;
        hp[4 + q] = h1;
        return true;
    }
    return hp[q] == h0 && hp[4 + q] == h1;
}

// MODE 0: encode, MODE 1: verify-decode.  Workgroup = one group of one object.
template <int MODE>
__global__ __launch_bounds__(TPB) void rag_group_kernel(const Obj *objs, const uint32_t *groups, uint32_t count,
                                                        uint8_t *hashes, uint32_t *status, uint8_t *gcv) {
    __shared__ __attribute__((aligned(16))) uint32_t cvs[2][S][8];     // a level and the next
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];  // each quad's message block
    const int t = threadIdx.x, q = t & 3, g = t >> 2;
    const uint32_t obj = find_obj(groups, count, blockIdx.x);
    const Obj a = objs[obj];
    const uint64_t grp = blockIdx.x - a.g0, N = a.N, n = a.n;
    const uint64_t c0 = grp * S, r = N - c0 < (uint64_t)S ? N - c0 : (uint64_t)S;  // my chunks
    const bool whole = N <= (uint64_t)S;           // the root is inside this group
    const bool from_src = MODE == 0 && a.C == 0;  // bao of the content: read it where it is
    uint8_t *const hash = hashes + 32 * (uint64_t)obj;
    bool ok = true;

    // ---- phase 1: the header; (encode, Bao only) the content into its chunk
    // slots; (decode) content bytes out
    if (MODE == 0) {
        if (grp == 0 && t == 0) *glb(reinterpret_cast<uint64_t *>(a.stream)) = n;
        if (from_src) {
            const uint64_t lim = n < (c0 + r) * 1024 ? n : (c0 + r) * 1024;
            for (uint64_t o = c0 * 1024 + 16 * (uint64_t)t; o < lim; o += 16 * TPB) {
                const u32x4 v = zf::load16_masked(a.src, o, n);
                uint8_t *p = a.stream + chunk_stream_off(o / 1024, N) + o % 1024;
                if (o + 16 <= lim) store16_a8<false>(p, v);
                else store16_partial(p, v, (uint32_t)(lim - o));
            }
        }
    } else {
        if (grp == 0 && t == 0 && *reinterpret_cast<const uint64_t *>(a.stream) != n) ok = false;
        const uint64_t lim = a.out_limit < (c0 + r) * 1024 ? a.out_limit : (c0 + r) * 1024;
        for (uint64_t o = c0 * 1024 + 16 * (uint64_t)t; o < lim; o += 16 * TPB) {
            const uint8_t *p = a.stream + chunk_stream_off(o / 1024, N) + o % 1024;
            const uint64_t left = lim - o;
            if (left >= 16) *glb(reinterpret_cast<u32x4 *>(a.out + o)) = load16_a8(p);
            else store16_partial(a.out + o, load16_partial(p, (uint32_t)left), (uint32_t)left);
        }
    }

    // ---- phase 2: chunk CVs, one quad per chunk
    const uint32_t slot = (uint32_t)(reinterpret_cast<uintptr_t>(&msg[g][0]) - reinterpret_cast<uintptr_t>(&msg[0][0]));
    const uint8_t *mbase = reinterpret_cast<const uint8_t *>(&msg[0][0]);
    const small::MsgIdx mi(q, slot);
    const uint32_t iv0 = q == 0 ? IV(0) : q == 1 ? IV(1) : q == 2 ? IV(2) : IV(3);
    const uint32_t iv1 = q == 0 ? IV(4) : q == 1 ? IV(5) : q == 2 ? IV(6) : IV(7);
    u32x4 stn[LOGS];  // decode: the stored nodes this quad checks, in flight with its chunk
    if ((uint64_t)g < r) {
        const uint64_t c = c0 + g;
        const uint64_t rem = n - c * 1024;  // n = 0: the empty chunk
        const uint32_t clen = rem < 1024 ? (uint32_t)rem : 1024u;
        const uint32_t nb = clen == 0 ? 1u : (clen + 63) / 64;
        const uint8_t *cp = a.stream + chunk_stream_off(c, N);
        if (MODE == 1) {
            uint64_t cp_ = r;
#pragma unroll
            for (int l = 1; l <= LOGS; ++l) {
                const uint64_t cn = (cp_ + 1) / 2;
                if ((uint64_t)g < cn && 2 * (uint64_t)g + 1 < cp_)
                    stn[l - 1] = load16_a8(a.stream + parent_stream_off(((c0 >> l) + g) << l, l, N) + 16 * q);
                cp_ = cn;
            }
        }
        u32x4 pc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) {  // my 16 B of every block of the chunk, all loads in flight
            const uint32_t off = 64 * b + 16 * q;
            if (off >= clen) pc[b] = u32x4{0u, 0u, 0u, 0u};
            else if (from_src) pc[b] = zf::load16_masked(a.src, c * 1024 + off, n);
            else pc[b] = off + 16 <= clen ? load16_a8(cp + off) : small::load16_bytes(cp + off, clen - off);
        }
        uint32_t h0 = iv0, h1 = iv1;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            if ((uint32_t)b < nb) {
                *reinterpret_cast<u32x4 *>(&msg[g][4 * q]) = pc[b];
                wave_sync();
                const bool lastb = (uint32_t)b + 1 == nb;
                const uint32_t flags = (b == 0 ? F_CHUNK_START : 0u) | (lastb ? F_CHUNK_END : 0u) |
                                       (lastb && N == 1 ? F_ROOT : 0u);
                small::compress4(h0, h1, mbase, mi, q, iv0, c, lastb ? clen - 64 * b : 64u, flags);
                wave_sync();
            }
        }
        if (N == 1) {  // the chunk is the root
            ok &= root_out<MODE>(hash, q, h0, h1);
        } else {
            cvs[0][g][q] = h0;
            cvs[0][g][4 + q] = h1;
        }
    }
    __syncthreads();

    // ---- phase 3: the group's levels 1 .. 6, one quad per parent
    int cur = 0;
    uint64_t cnt_prev = r;
    for (int level = 1; level <= LOGS && cnt_prev > 1; ++level) {
        const uint64_t cnt = (cnt_prev + 1) / 2;
        if ((uint64_t)g < cnt) {
            const uint64_t p = g;
            if (2 * p + 1 >= cnt_prev) {  // odd last node: promoted unchanged
                cvs[cur ^ 1][p][q] = cvs[cur][2 * p][q];
                cvs[cur ^ 1][p][4 + q] = cvs[cur][2 * p][4 + q];
            } else {
                const u32x4 mw = *reinterpret_cast<const u32x4 *>(&cvs[cur][2 * p + (q >> 1)][4 * (q & 1)]);
                *reinterpret_cast<u32x4 *>(&msg[g][4 * q]) = mw;
                wave_sync();
                const bool root = whole && cnt == 1;
                uint32_t h0 = iv0, h1 = iv1;
                small::compress4(h0, h1, mbase, mi, q, iv0, 0, 64, F_PARENT | (root ? F_ROOT : 0u));
                wave_sync();
                if (MODE == 0) {
                    store16_a8<false>(a.stream + parent_stream_off(((c0 >> level) + p) << level, level, N) + 16 * q, mw);
                } else {
                    u32x4 s = stn[0];
#pragma unroll
                    for (int l = 2; l <= LOGS; ++l)
                        if (level == l) s = stn[l - 1];
                    ok &= s.x == mw.x && s.y == mw.y && s.z == mw.z && s.w == mw.w;
                }
                if (root) {
                    ok &= root_out<MODE>(hash, q, h0, h1);
                } else {
                    cvs[cur ^ 1][p][q] = h0;
                    cvs[cur ^ 1][p][4 + q] = h1;
                }
            }
        }
        __syncthreads();
        cur ^= 1;
        cnt_prev = cnt;
    }
    if (MODE == 1 && !ok) flag_mismatch(status, obj);

    // ---- phase 4: the group's CV for the top kernel
    if (!whole && t < 8) *glb(reinterpret_cast<uint32_t *>(gcv + 32 * (uint64_t)blockIdx.x) + t) = cvs[cur][0][t];
}

// Workgroup = one object: levels 7 .. root over its G > 1 group CVs, a quad per
// parent; decode checks the top's stored nodes, staged in LDS up front.
template <int MODE>
__global__ __launch_bounds__(TPB) void rag_top_kernel(const Obj *objs, const uint32_t *groups, uint8_t *hashes,
                                                      uint32_t *status, const uint8_t *gcv) {
    __shared__ __attribute__((aligned(16))) uint32_t cv[2][GMAX][8];
    __shared__ __attribute__((aligned(16))) uint32_t msg[QUADS][16];
    __shared__ __attribute__((aligned(16))) u32x4 stored[MODE == 1 ? GMAX * 4 : 4];
    const int t = threadIdx.x, q = t & 3, g = t >> 2;
    const uint32_t obj = blockIdx.x, g0 = groups[obj];
    const uint64_t G = groups[obj + 1] - g0;
    if (G <= 1) return;  // the group kernel finished this object (uniform over the workgroup)
    const Obj a = objs[obj];
    const uint64_t N = a.N;
    const uint32_t *mine = reinterpret_cast<const uint32_t *>(gcv + 32 * (uint64_t)g0);
    for (uint64_t i = t; i < 8 * G; i += TPB) cv[0][i >> 3][i & 7] = mine[i];
    if (MODE == 1) {  // level by level: pairs floor(cnt / 2), 16 B per lane of a quad
        uint64_t cnt = G, base = 0;
        for (int level = LOGS + 1; cnt > 1; ++level) {
            const uint64_t pairs = cnt / 2;
            for (uint64_t i = t; i < 4 * pairs; i += TPB)
                stored[4 * base + i] = load16_a8(a.stream + parent_stream_off((i >> 2) << level, level, N) + 16 * (i & 3));
            base += pairs;
            cnt = (cnt + 1) / 2;
        }
    }
    __syncthreads();
    const uint32_t slot = (uint32_t)(reinterpret_cast<uintptr_t>(&msg[g][0]) - reinterpret_cast<uintptr_t>(&msg[0][0]));
    const uint8_t *mbase = reinterpret_cast<const uint8_t *>(&msg[0][0]);
    const small::MsgIdx mi(q, slot);
    const uint32_t iv0 = q == 0 ? IV(0) : q == 1 ? IV(1) : q == 2 ? IV(2) : IV(3);
    const uint32_t iv1 = q == 0 ? IV(4) : q == 1 ? IV(5) : q == 2 ? IV(6) : IV(7);
    uint8_t *const hash = hashes + 32 * (uint64_t)obj;
    uint64_t nbase = 0;  // decode: index of this level's first node in `stored`
    int cur = 0;
    uint64_t cnt_prev = G;
    bool ok = true;
    for (int level = LOGS + 1; cnt_prev > 1; ++level) {
        const uint64_t cnt = (cnt_prev + 1) / 2;
        for (uint64_t p = g; p < cnt; p += QUADS) {
            if (2 * p + 1 >= cnt_prev) {  // odd last node: promoted unchanged
                cv[cur ^ 1][p][q] = cv[cur][2 * p][q];
                cv[cur ^ 1][p][4 + q] = cv[cur][2 * p][4 + q];
                continue;
            }
            const u32x4 mw = *reinterpret_cast<const u32x4 *>(&cv[cur][2 * p + (q >> 1)][4 * (q & 1)]);
            *reinterpret_cast<u32x4 *>(&msg[g][4 * q]) = mw;
            wave_sync();
            const bool root = cnt == 1;
            uint32_t h0 = iv0, h1 = iv1;
            small::compress4(h0, h1, mbase, mi, q, iv0, 0, 64, F_PARENT | (root ? F_ROOT : 0u));
            wave_sync();
            if (MODE == 0) {
                store16_a8<false>(a.stream + parent_stream_off(p << level, level, N) + 16 * q, mw);
            } else {
                const u32x4 s = stored[4 * (nbase + p) + q];
                ok &= s.x == mw.x && s.y == mw.y && s.z == mw.z && s.w == mw.w;
            }
            if (root) {
                ok &= root_out<MODE>(hash, q, h0, h1);
            } else {
                cv[cur ^ 1][p][q] = h0;
                cv[cur ^ 1][p][4 + q] = h1;
            }
        }
        __syncthreads();
        cur ^= 1;
        nbase += cnt_prev / 2;
        cnt_prev = cnt;
    }
    if (MODE == 1 && !ok) flag_mismatch(status, obj);
}

}  // namespace ragged

hipError_t ragged_launch(const RaggedLaunch &L, hipStream_t stream) {
    using namespace ragged;
    const uint32_t count = (uint32_t)L.count;
    if (L.parity_blocks) {  // Zfec bit, encode
        const void *tab = nullptr;
        const hipError_t e = zfec_parity_table(4, 8, &tab);
        if (e != hipSuccess) return e;
        const auto k = L.bao ? rag_parity_kernel<1> : rag_parity_kernel<0>;
        hipLaunchKernelGGL(k, dim3((unsigned)L.parity_blocks), dim3(TPB), 0, stream, L.objs, L.blocks, count,
                           static_cast<const uint32_t *>(tab));
    }
    if (L.copy_blocks)  // Zfec only, decode
        hipLaunchKernelGGL(rag_copy_kernel, dim3((unsigned)L.copy_blocks), dim3(TPB), 0, stream, L.objs, L.blocks, count);
    if (L.bao && L.total_groups) {
        const auto kg = L.decode ? rag_group_kernel<1> : rag_group_kernel<0>;
        hipLaunchKernelGGL(kg, dim3((unsigned)L.total_groups), dim3(TPB), 0, stream, L.objs, L.groups, count, L.hashes,
                           L.status, L.gcv);
        if (L.total_groups > L.count) {  // some object has more than one group
            const auto kt = L.decode ? rag_top_kernel<1> : rag_top_kernel<0>;
            hipLaunchKernelGGL(kt, dim3(count), dim3(TPB), 0, stream, L.objs, L.groups, L.hashes, L.status, L.gcv);
        }
    }
    return hipGetLastError();
}

}  // namespace chip
