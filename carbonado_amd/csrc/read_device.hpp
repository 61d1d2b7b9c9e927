// read_device.hpp — device functions the ranged reads (read_kernels.hip, KD)
// share with the vouched ranged reads (vread_kernels.hip, KV).
#pragma once

#include "audit_checks.hpp"
#include "read_plan.hpp"

namespace chip {
namespace read {

// A segment's own slice is authentic.  KD keeps one status word per slice; KV
// splits the own slice's into a chunk word (rstat[g]) and a path word, and
// either one set condemns it (PATH).
template <bool PATH>
__device__ __forceinline__ bool own_ok(const uint32_t *rstat, const uint32_t *pathw, uint32_t g) {
    return (PATH ? rstat[g] | pathw[g] : rstat[g]) == 0;
}

// How segment g is served: direct when its own slice is authentic, else rebuilt
// from the four lowest authentic shares among its 7 fallback words (the mask's
// entry of the host-built table, row p of their inverse), else failed.
template <bool PATH>
__device__ __forceinline__ Served serve_segment(const Seg *segs, const MaskEntry *masks, const uint32_t *rstat,
                                                const uint32_t *pathw, uint32_t nseg, uint32_t g) {
    Served out = {DIRECT, 0u, 0u, 0u};
    if (own_ok<PATH>(rstat, pathw, g)) return out;
    const uint32_t p = segs[g].p;
    uint32_t mask = 0;
    for (uint32_t i = 0; i < M; ++i)
        if (i != p && rstat[nseg + FALLBACKS * g + (i < p ? i : i - 1)] == 0) mask |= 1u << i;
    const MaskEntry *e = masks + mask;  // read in place: no private copy indexed by p
    if (!e->ok) {
        out.mode = FAILED;
        return out;
    }
    out.mode = REBUILT;
    for (uint32_t s = 0; s < K; ++s) {
        out.sel |= (uint32_t)e->sel[s] << (8 * s);
        out.coef |= (uint32_t)e->coef[K * p + s] << (8 * s);
    }
    return out;
}

// segment g's own slice request moved to fallback k of its 7 (shard k below its primary p, k + 1 from it on)
__device__ __forceinline__ audit::Req fallback_slice(audit::Req a, const Seg *segs, uint32_t g, uint32_t k) {
    const uint32_t p = segs[g].p, spc = segs[g].spc, shard = k < p ? k : k + 1;
    const uint64_t first = (uint64_t)shard * spc + (a.first - (uint64_t)p * spc);
    a.last = first + (a.last - a.first);
    a.first = first;
    return a;
}

// Fallback parent item i of segment g, behind the caller's gate: items
// [fpar[g], fpar[g + 1]) are the segment's, 7 x the most parents any of its
// fallback slices selects; a mismatch flags the slice's word of rstat.
__device__ __forceinline__ void fallback_parent_item(const audit::Req *slices, const Seg *segs, const uint64_t *fpar,
                                                     uint32_t nseg, uint64_t i, uint32_t g, uint32_t *rstat) {
    const uint64_t local = i - fpar[g], each = (fpar[g + 1] - fpar[g]) / FALLBACKS;
    const uint32_t k = (uint32_t)(local / each);
    const audit::Req a = fallback_slice(slices[g], segs, g, k);
    const uint64_t j = local % each;
    if (j >= audit::sel_parents(a.N, a.first, a.last)) return;  // this slice selects fewer
    if (!audit::parent_ok<false>(a, j)) bao::flag_mismatch(rstat, nseg + FALLBACKS * g + k);
}

// Fallback chunk item i of segment g on the quad of lane t, behind the
// caller's gate: items [7 pre[g], 7 pre[g + 1]) are the segment's, pre = KA's
// chunk prefix of the primary slices.
__device__ __forceinline__ void fallback_chunk_item(const audit::Req *slices, const Seg *segs, const uint64_t *pre,
                                                    uint32_t nseg, uint64_t i, uint32_t g, uint32_t *rstat,
                                                    uint32_t (&msg)[audit::QUADS][16], int t) {
    const uint64_t local = i - FALLBACKS * pre[g], each = pre[g + 1] - pre[g];
    const uint32_t k = (uint32_t)(local / each);
    const audit::Req a = fallback_slice(slices[g], segs, g, k);
    if (!audit::chunk_ok<false>(a, local % each, msg, t)) bao::flag_mismatch(rstat, nseg + FALLBACKS * g + k);
}

}  // namespace read
}  // namespace chip
