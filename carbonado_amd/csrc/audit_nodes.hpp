// audit_nodes.hpp — the nodes of a slice request by arithmetic, compiled by the
// kernels of audit_kernels.hip and by the host (audit_plan.hpp, and the
// stand-alone tests/audit_plan_check.cpp, which enumerates every request's
// work items through these functions): no HIP type in it.
//
// The tree over N chunks in levels: level 0 = the chunks, level L has
// cnt_L = ceil(cnt_{L-1} / 2) nodes, of which the first np_L = floor(cnt_{L-1} / 2)
// are parents (two children) and an odd last one is the promoted node of the
// level below.  Parent (L, q) has leftmost chunk q << L and covers chunks
// [q << L, min((q + 1) << L, N)).  A request selects chunks [f, l), f < l <= N,
// and with them every parent whose cover meets [f, l): at level L those are
// q in [f >> L, min((l - 1) >> L, np_L - 1)].
//
// A node is (level lv, leftmost chunk s); its bytes sit
//  * in the stream at 8 + 1024 s + 64 (P(s) + c(s) - lv), P(s) = parents whose
//    leftmost chunk is < s, c(s) = parents whose leftmost chunk is s
//    (bao_device.hpp: parents_before, parents_at), and
//  * in the request's proof (header, then the selected nodes in pre-order) at
//    8 + 1024 max(s - f, 0) + 64 (Psel(s) + c(s) - lv), Psel(s) = SELECTED
//    parents whose leftmost chunk is < s: every parent above a selected node
//    with the same leftmost chunk is selected too, and of the selected chunks
//    only the last one of the stream can be short.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define AUDIT_HD __host__ __device__ __forceinline__
#else
#define AUDIT_HD inline
#endif

namespace chip {
namespace audit {

AUDIT_HD int clog2(uint64_t x) { return x <= 1 ? 0 : 64 - __builtin_clzll(x - 1); }  // x >= 1

AUDIT_HD uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }

// The owner of work item i in a prefix array: pre[r] <= i < pre[r + 1]
// (pre[0] = 0, pre[count] > i; owners without items are passed over).  Every
// kernel that finds its request, segment or repair by its index goes through
// this, and so does the host where it enumerates the same items.
template <typename T>
AUDIT_HD uint32_t prefix_find(const T *pre, uint32_t count, T i) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// c(s)
AUDIT_HD int parents_at(uint64_t s, uint64_t N) {
    const int cl = clog2(N - s);
    if (s == 0) return cl;
    const int tz = __builtin_ctzll(s);
    return tz < cl ? tz : cl;
}

// selected parents of (N, f, l) whose leftmost chunk is < s (f = 0, l = N: P(s))
AUDIT_HD uint64_t sel_parents_before(uint64_t s, uint64_t N, uint64_t f, uint64_t l) {
    uint64_t total = 0, cnt = N;
    for (int L = 1; cnt > 1; ++L) {
        const uint64_t np = cnt / 2, qlo = f >> L;
        const uint64_t end = umin(umin(((l - 1) >> L) + 1, np), (s + (1ull << L) - 1) >> L);  // q < end
        if (end > qlo) total += end - qlo;
        cnt = (cnt + 1) / 2;
    }
    return total;
}

// selected parents of (N, f, l), all levels
AUDIT_HD uint64_t sel_parents(uint64_t N, uint64_t f, uint64_t l) {
    uint64_t total = 0, cnt = N;
    for (int L = 1; cnt > 1; ++L) {
        const uint64_t np = cnt / 2, qlo = f >> L, end = umin(((l - 1) >> L) + 1, np);
        if (end > qlo) total += end - qlo;
        cnt = (cnt + 1) / 2;
    }
    return total;
}

// the k-th selected parent (level order, k < sel_parents): its level, its
// leftmost chunk to *s
AUDIT_HD int parent_item(uint64_t N, uint64_t f, uint64_t l, uint64_t k, uint64_t *s) {
    uint64_t cnt = N;
    for (int L = 1; cnt > 1; ++L) {
        const uint64_t np = cnt / 2, qlo = f >> L, end = umin(((l - 1) >> L) + 1, np);
        const uint64_t here = end > qlo ? end - qlo : 0;
        if (k < here) {
            *s = (qlo + k) << L;
            return L;
        }
        k -= here;
        cnt = (cnt + 1) / 2;
    }
    *s = 0;
    return 0;  // not reached for k < sel_parents
}

AUDIT_HD bool is_root(uint64_t s, int lv, uint64_t N) { return s == 0 && (lv >= 63 || (1ull << lv) >= N); }

// Nearest real parent above node (lv, sx): the lowest level lp > lv whose node
// containing sx has two children; 0 when the node is the root.  The node is
// that parent's left child iff sx is the parent's leftmost chunk.
AUDIT_HD int nearest_parent(uint64_t sx, int lv, uint64_t N, uint64_t *sp) {
    for (int lp = lv + 1; lp < 64; ++lp) {
        const uint64_t s0 = (sx >> lp) << lp;
        if (s0 + (1ull << (lp - 1)) < N) {
            *sp = s0;
            return lp;
        }
        if (s0 == 0 && (1ull << lp) >= N) return 0;
    }
    return 0;
}

// byte offset of node (lv, s) in the stream
AUDIT_HD uint64_t stream_off(uint64_t s, int lv, uint64_t N) {
    return 8 + 1024 * s + 64 * (sel_parents_before(s, N, 0, N) + (uint64_t)(parents_at(s, N) - lv));
}

// byte offset of the selected node (lv, s) in the proof of (N, f, l)
AUDIT_HD uint64_t proof_off(uint64_t s, int lv, uint64_t N, uint64_t f, uint64_t l) {
    return 8 + 1024 * (s > f ? s - f : 0) + 64 * (sel_parents_before(s, N, f, l) + (uint64_t)(parents_at(s, N) - lv));
}

// Where a node's bytes are read: in the stream, or in the request's proof.
template <bool PROOF>
AUDIT_HD uint64_t node_off(uint64_t s, int lv, uint64_t N, uint64_t f, uint64_t l) {
    return PROOF ? proof_off(s, lv, N, f, l) : stream_off(s, lv, N);
}

// Offset (same addressing) of the 32 bytes node (lv, s) is checked against:
// its half of its nearest parent.  Not for the root.
template <bool PROOF>
AUDIT_HD uint64_t slot_off(uint64_t s, int lv, uint64_t N, uint64_t f, uint64_t l) {
    uint64_t sp = 0;
    const int lp = nearest_parent(s, lv, N, &sp);
    return node_off<PROOF>(sp, lp, N, f, l) + (s == sp ? 0 : 32);
}

// bytes of chunk c of n content bytes (n = 0: the empty chunk)
AUDIT_HD uint64_t chunk_len(uint64_t c, uint64_t n) { return n - c * 1024 < 1024 ? n - c * 1024 : 1024; }

}  // namespace audit
}  // namespace chip
