// stream_rules.hpp — the rules every plan header and api_*.cpp takes from one
// place: the geometry of a bao stream, rounding, the overlap check of a call's
// output ranges, the zfec padding rule and scrub's verdicts behind the shard
// mask.  Pure host code without a HIP type in it: the stand-alone check
// programs under tests/ compile it with the plan headers under a sanitizer.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/carbonado_hip.h"

#if defined(__HIPCC__)
#define RULES_HD __host__ __device__ inline  // also compiled by the kernel that plans reads (qread_kernels.hip)
#else
#define RULES_HD inline
#endif

namespace chip {
namespace rules {

// ---- an Ecies envelope -----------------------------------------------------------
constexpr uint64_t ENV_OVERHEAD = 97;  // eph_pub65 || nonce16 || tag16 in front of the ciphertext

// ---- a bao stream of n content bytes ------------------------------------------
RULES_HD uint64_t chunks(uint64_t n) { return n == 0 ? 1 : (n + 1023) / 1024; }
inline uint64_t bao_len(uint64_t n) { return 8 + n + 64 * (chunks(n) - 1); }

// content length of a bao stream of `len` bytes (bao_len is strictly
// increasing); false: no such stream
inline bool bao_content(uint64_t len, uint64_t *n) {
    if (len < 8) return false;
    uint64_t lo = 0, hi = len - 8;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (bao_len(mid) < len) lo = mid + 1;
        else hi = mid;
    }
    *n = lo;
    return bao_len(lo) == len;
}

// ---- rounding -----------------------------------------------------------------
inline uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
inline uint64_t up16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

// true when two of the ranges [off[r], off[r] + len[r]) with len[r] > 0 share a
// byte (ranges that touch do not)
inline bool ranges_overlap(const uint64_t *off, const uint64_t *len, uint64_t count) {
    // ranges in ascending order (what the layout calls hand out) need one pass and no sort
    uint64_t end = 0, o = 0;
    for (; o < count; ++o) {
        if (!len[o]) continue;
        if (off[o] < end) break;
        end = off[o] + len[o];
    }
    if (o == count) return false;
    std::vector<std::pair<uint64_t, uint64_t>> r;
    r.reserve(count);
    for (o = 0; o < count; ++o)
        if (len[o]) r.emplace_back(off[o], len[o]);
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i - 1].first + r[i - 1].second > r[i].first) return true;
    return false;
}

// ---- zfec ------------------------------------------------------------------------
// utils.rs:47-58, k generalised: n bytes are padded to a multiple of 1024 k and
// cut into k shards of C bytes
struct Pad {
    uint32_t pad;
    uint64_t C;
};
inline Pad calc_pad(uint64_t n, uint32_t k) {
    const uint64_t target = up(n, 1024ull * k);
    return {(uint32_t)(target - n), target / k};
}

// What scrub decides for a stream of `len` bytes with shard length C from the
// number of its authentic shares, behind the checks each caller makes first
// (decoding.rs:187-203): a status, or REPAIR.
constexpr int REPAIR = -1;
inline int scrub_verdict(uint64_t len, uint64_t C, uint32_t padding, uint32_t good) {
    if (good < CHIP_FEC_K) return CHIP_ERR_ZFEC;  // zfec_chunks: too few shares
    const uint64_t kc = (uint64_t)CHIP_FEC_K * C;
    if (padding > kc) return CHIP_ERR_ZFEC;
    const Pad again = calc_pad(kc - padding, CHIP_FEC_K);  // of the decoded object, as the re-encode pads it
    if (again.pad != padding) return CHIP_ERR_SCRUBBED_PADDING_MISMATCH;             // decoding.rs:192-194
    if (bao_len(CHIP_FEC_M * again.C) != len) return CHIP_ERR_SCRUBBED_LENGTH_MISMATCH;  // decoding.rs:198-203
    return REPAIR;
}

}  // namespace rules
}  // namespace chip
