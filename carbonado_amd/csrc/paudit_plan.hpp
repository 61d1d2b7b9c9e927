// paudit_plan.hpp — host side of the device-planned slice audits
// (include/carbonado_hip_paudit.h): the auditor's root table and its one
// upload, and the O(1) host work of a call (argument checks in the header's
// order, grid bounds, scratch layout).  The requests themselves are planned on
// the device (paudit_device.hpp, paudit_kernels.hip); the host never sees them,
// so every grid of a call is a BOUND from (info, nreq, max_count), not a total.
// Pure host code without a HIP type in it (tests/paudit_plan_check.cpp drives it
// under a sanitizer).
#pragma once

#include <cstring>

#include "../../include/carbonado_hip_paudit.h"
#include "paudit_device.hpp"
#include "qread_plan.hpp"

namespace chip {
namespace paudit {

using audit::up;

static_assert(NO_REQUEST == CHIPP_NO_REQUEST, "one spare value");

// ---- the root table ----------------------------------------------------------------
// nroots records, StreamRec with src = 0, C = 0 and padding = 0.
inline uint64_t root_table_len(uint64_t nroots) {
    if (nroots >= (1ull << 32)) return 0;  // a request names its stream in 32 bits
    return up(nroots * sizeof(StreamRec), 256);
}

// The host checks of chipp_root_table_dev, in the header's order, and the table
// as uploaded.  Addresses are plain integers here.
inline int plan_root_table(const uint64_t *content_len, uintptr_t d_hash, uint64_t nroots, uintptr_t d_table,
                           uint64_t table_len_given, chipp_root_info *info, std::vector<uint8_t> *table) {
    if (!info) return CHIP_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    if (nroots && !content_len) return CHIP_ERR_INVALID_ARG;
    if (!d_table || d_table % 16 || nroots >= (1ull << 32)) return CHIP_ERR_INVALID_ARG;
    for (uint64_t s = 0; s < nroots; ++s)
        if (content_len[s] > audit::MAX_CONTENT) return CHIP_ERR_INVALID_ARG;
    if (table_len_given < root_table_len(nroots)) return CHIP_ERR_INVALID_ARG;
    if (!d_hash) return CHIP_ERR_HASH_DECODE;
    table->assign(root_table_len(nroots), 0);
    StreamRec *recs = reinterpret_cast<StreamRec *>(table->data());
    info->nroots = nroots;
    for (uint64_t s = 0; s < nroots; ++s) {
        StreamRec &q = recs[s];
        q.src = 0;
        q.n = content_len[s];
        q.N = audit::chunks(content_len[s]);
        q.hash = d_hash + 32 * s;
        q.C = 0;
        q.padding = 0;
        info->max_chunks = std::max<uint64_t>(info->max_chunks, q.N);
    }
    return CHIP_OK;
}

// ---- grid bounds --------------------------------------------------------------------
inline bool count_ok(uint64_t max_count) { return max_count != 0 && max_count <= audit::MAX_SLICE; }

// 8 + 64 P + 1024 max_count (max_count <= 2^53: nothing wraps)
inline uint64_t proof_bound(uint64_t max_chunks, uint64_t max_count) {
    if (!count_ok(max_count)) return 0;
    return 8 + 64 * qread::slice_parents_bound(max_chunks, max_count) + 1024 * max_count;
}

struct Geometry {
    uint64_t W = 0;  // chunk slots per request: no request selects more chunks than its stream has
    uint64_t P = 0;  // parent slots per request: qread::slice_parents_bound(max_chunks, W)
    // work items of a call: lanes of the parent check, quads of the chunk check, 16-B units of the gathers
    uint64_t parents = 0, chunks = 0, content_units = 0, extract_units = 0;
    bool ok = false;  // every bound below 2^36 items (so below 2^31 workgroups)
    Geometry() {}
    Geometry(uint64_t max_chunks, uint64_t nreq, uint64_t max_count) {
        W = audit::umin(max_count, std::max<uint64_t>(max_chunks, 1));
        P = qread::slice_parents_bound(max_chunks, W);
        const unsigned __int128 one = 1;
        const unsigned __int128 par = one * nreq * P, chk = one * nreq * W, cu = 64 * chk,
                                eu = one * nreq * (1 + 4 * P) + cu;
        ok = par < audit::MAX_ITEMS && cu < audit::MAX_ITEMS && eu < audit::MAX_ITEMS;
        if (!ok) return;
        parents = (uint64_t)par; chunks = (uint64_t)chk; content_units = (uint64_t)cu; extract_units = (uint64_t)eu;
    }
};

// ---- the scratch ------------------------------------------------------------------
// [requests (audit::Req) | parent count per request], each on a 256-B boundary.
struct ScratchLayout {
    uint64_t reqs = 0, parents = 0, total = 0;
    ScratchLayout() {}
    explicit ScratchLayout(uint64_t nreq) {
        parents = up(nreq * sizeof(audit::Req), 256);
        total = parents + up(nreq * 8, 256);
    }
};

inline uint64_t scratch_len(uint64_t max_chunks, uint64_t nreq, uint64_t max_count) {
    if (nreq >= (1ull << 31) || !count_ok(max_count)) return 0;
    return Geometry(max_chunks, nreq, max_count).ok ? ScratchLayout(nreq).total : 0;
}

// One output buffer of a call: slot r at base + r stride.
struct Slots {
    bool used;
    uintptr_t base;
    uint64_t stride, min_stride;
};
inline bool stride_ok(const Slots &s, uint64_t nreq) {
    return !s.used || (s.stride % 16 == 0 && s.stride >= s.min_stride && s.stride <= (~0ull - s.base) / nreq);
}

// The host checks of a call, in the header's order; everything but the device.
// have_pointers: every pointer of the call's signature is there.
inline int plan_call(bool have_pointers, uintptr_t d_table, uint64_t max_chunks, uint64_t nreq, uint64_t max_count,
                     bool with_content, uintptr_t d_content, uint64_t content_stride, bool with_proofs,
                     uintptr_t d_proofs, uint64_t proof_stride, uintptr_t d_scratch, uint64_t scratch_len_given,
                     Geometry *g, ScratchLayout *lay) {
    if (nreq == 0) return CHIP_OK;
    if (!have_pointers) return CHIP_ERR_INVALID_ARG;
    if (nreq >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    if (!count_ok(max_count)) return CHIP_ERR_INVALID_ARG;
    const Slots content{with_content, d_content, content_stride, 1024 * max_count};
    const Slots proofs{with_proofs, d_proofs, proof_stride, proof_bound(max_chunks, max_count)};
    if (!stride_ok(content, nreq) || !stride_ok(proofs, nreq)) return CHIP_ERR_INVALID_ARG;
    if ((with_content && d_content % 16) || (with_proofs && d_proofs % 16) || d_table % 16 || d_scratch % 16)
        return CHIP_ERR_INVALID_ARG;
    *g = Geometry(max_chunks, nreq, max_count);
    if (!g->ok) return CHIP_ERR_INVALID_ARG;
    *lay = ScratchLayout(nreq);
    if (scratch_len_given < lay->total) return CHIP_ERR_INVALID_ARG;
    return CHIP_OK;
}

}  // namespace paudit
}  // namespace chip
