// audit_checks.hpp — the per-node checks of a slice request as device
// functions, shared by KA (audit_kernels.hip) and the gated checks of the
// ranged reads (read_kernels.hip): a work item's request by binary search in a
// prefix array, one selected parent on a lane, one selected chunk on a quad of
// lanes (quad_b3.hpp).  The kernels around them decide which items run and
// what a mismatch flags.
#pragma once

#include <hip/hip_runtime.h>

#include "audit_plan.hpp"
#include "bao_device.hpp"
#include "chip_internal.hpp"
#include "quad_b3.hpp"

namespace chip {
namespace audit {

using namespace bao;

constexpr int TPB = 256, QUADS = TPB / 4;

__device__ __forceinline__ uint32_t hash_word(const uint8_t *h, int w) {  // any alignment
    return (uint32_t)h[4 * w] | (uint32_t)h[4 * w + 1] << 8 | (uint32_t)h[4 * w + 2] << 16 |
           (uint32_t)h[4 * w + 3] << 24;
}

// the k-th selected parent of request a, on one lane: b3_parent of its 64
// stored bytes against the CV stored in its own parent (the root: the hash)
template <bool PROOF>
__device__ __forceinline__ bool parent_ok(const Req &a, uint64_t k) {
    uint64_t s = 0;
    const int lv = parent_item(a.N, a.first, a.last, k, &s);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    const uint8_t *node = src + node_off<PROOF>(s, lv, a.N, a.first, a.last);
    uint32_t l[8], rr[8], cv[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const u32x2 x = reinterpret_cast<const u32x2 *>(node)[w];
        const u32x2 y = reinterpret_cast<const u32x2 *>(node + 32)[w];
        l[2 * w] = x.x; l[2 * w + 1] = x.y; rr[2 * w] = y.x; rr[2 * w + 1] = y.y;
    }
    const bool root = is_root(s, lv, a.N);
    b3_parent(l, rr, root, cv);
    bool ok = true;
    if (root) {
        const uint8_t *h = reinterpret_cast<const uint8_t *>(a.hash);
#pragma unroll
        for (int w = 0; w < 8; ++w) ok &= hash_word(h, w) == cv[w];
    } else {
        const uint8_t *slot = src + slot_off<PROOF>(s, lv, a.N, a.first, a.last);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u32x2 x = reinterpret_cast<const u32x2 *>(slot)[w];
            ok &= x.x == cv[2 * w] && x.y == cv[2 * w + 1];
        }
    }
    return ok;
}

// the k-th selected chunk of request a, on the quad of lane t (quad t >> 2 of
// the workgroup, msg = each quad's message block in LDS): its 16 blocks
// compressed in a chain, the CV against the one stored in its parent (a
// one-chunk stream: the hash); the first chunk's quad checks the header.  No
// workgroup barrier: a whole quad may stay away.
template <bool PROOF>
__device__ __forceinline__ bool chunk_ok(const Req &a, uint64_t k, uint32_t (&msg)[QUADS][16], int t) {
    const int q = t & 3, g = t >> 2;
    const uint64_t c = a.first + k, N = a.N, n = a.n;
    const uint32_t clen = (uint32_t)chunk_len(c, n);  // n = 0: the empty chunk
    const uint32_t nb = clen == 0 ? 1u : (clen + 63) / 64;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(a.src);
    const uint8_t *cp = src + node_off<PROOF>(c, 0, N, a.first, a.last);
    bool ok = true;
    if (c == a.first && q == 0 && *reinterpret_cast<const uint64_t *>(src) != n) ok = false;  // the header

    const uint32_t slot = (uint32_t)(reinterpret_cast<uintptr_t>(&msg[g][0]) - reinterpret_cast<uintptr_t>(&msg[0][0]));
    const uint8_t *mbase = reinterpret_cast<const uint8_t *>(&msg[0][0]);
    const small::MsgIdx mi(q, slot);
    const uint32_t iv0 = q == 0 ? IV(0) : q == 1 ? IV(1) : q == 2 ? IV(2) : IV(3);
    const uint32_t iv1 = q == 0 ? IV(4) : q == 1 ? IV(5) : q == 2 ? IV(6) : IV(7);
    u32x4 pc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) {  // my 16 B of every block of the chunk, all loads in flight
        const uint32_t off = 64 * b + 16 * q;
        if (off >= clen) pc[b] = u32x4{0u, 0u, 0u, 0u};
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
        const uint8_t *h = reinterpret_cast<const uint8_t *>(a.hash);
        ok &= hash_word(h, q) == h0 && hash_word(h, 4 + q) == h1;
    } else {
        const uint32_t *want = reinterpret_cast<const uint32_t *>(src + slot_off<PROOF>(c, 0, N, a.first, a.last));
        ok &= want[q] == h0 && want[4 + q] == h1;
    }
    return ok;
}

}  // namespace audit
}  // namespace chip
