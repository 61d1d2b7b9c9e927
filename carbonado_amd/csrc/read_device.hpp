// read_device.hpp — device functions the ranged reads (read_kernels.hip, KD)
// share with the vouched ranged reads (vread_kernels.hip, KV).
#pragma once

#include "audit_checks.hpp"
#include "read_plan.hpp"

namespace chip {
namespace read {

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
