// audit_checks.hpp — what a slice audit does with one work item of a request,
// as device functions: one selected parent on a lane, one selected chunk on a
// quad of lanes (quad_b3.hpp), shared by KA (audit_kernels.hip), KB
// (paudit_kernels.hip) and the gated checks of the ranged reads
// (read_kernels.hip, vread_kernels.hip, qread_kernels.hip); 16 B of the
// content and of the proof gather on a lane, shared by KA and KB.  The kernels
// around them find a work item's request (a prefix search, slot arithmetic)
// and decide which items run and what a mismatch flags.
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

// ---- the gathers, 16 B per lane ---------------------------------------------------
// content bytes [o, o + 16) of request a (o < a.olen, 16 | o), the last unit
// short: the verified bytes where the request's status word stayed 0, zeros
// otherwise.  Content starts at the first selected chunk; 16 | 1024: a unit
// sits in one chunk.
template <bool PROOF>
__device__ __forceinline__ void content_unit(const Req &a, uint64_t o, uint32_t status) {
    const uint64_t left = a.olen - o;
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.dst) + o;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (status == 0) {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(a.src) +
                           node_off<PROOF>(a.first + o / 1024, 0, a.N, a.first, a.last) + o % 1024;
        v = left >= 16 ? load16_a8(p) : load16_partial(p, (uint32_t)left);
    }
    if (left >= 16) *glb(reinterpret_cast<u32x4 *>(dst)) = v;
    else store16_partial(dst, v, (uint32_t)left);
}

// the proof of request a, from its stream into its packed pre-order: the
// length header as stored, 16-B unit q < 4 of the k-th selected parent, 16-B
// unit q < 64 of the k-th selected chunk (nothing past a short last chunk)
__device__ __forceinline__ void proof_header(const Req &a) {
    *glb(reinterpret_cast<uint64_t *>(a.dst)) = *reinterpret_cast<const uint64_t *>(a.src);
}
__device__ __forceinline__ void proof_parent_unit(const Req &a, uint64_t k, uint64_t q) {
    uint64_t s = 0;
    const int lv = parent_item(a.N, a.first, a.last, k, &s);
    const uint64_t w = 16 * q;
    store16_a8<false>(reinterpret_cast<uint8_t *>(a.dst) + proof_off(s, lv, a.N, a.first, a.last) + w,
                      load16_a8(reinterpret_cast<const uint8_t *>(a.src) + stream_off(s, lv, a.N) + w));
}
__device__ __forceinline__ void proof_chunk_unit(const Req &a, uint64_t k, uint64_t q) {
    const uint64_t c = a.first + k, w = 16 * q, clen = chunk_len(c, a.n);
    if (w >= clen) return;  // past a short last chunk
    const uint8_t *p = reinterpret_cast<const uint8_t *>(a.src) + stream_off(c, 0, a.N) + w;
    uint8_t *d = reinterpret_cast<uint8_t *>(a.dst) + proof_off(c, 0, a.N, a.first, a.last) + w;
    if (w + 16 <= clen) store16_a8<false>(d, load16_a8(p));
    else store16_partial(d, load16_partial(p, (uint32_t)(clen - w)), (uint32_t)(clen - w));
}

}  // namespace audit
}  // namespace chip
