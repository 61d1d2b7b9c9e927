// audit_plan.hpp — host side of the slice audits (include/carbonado_hip_audit.h):
// argument checks, the caller's proof / content layout, and the per-request
// table the kernels of audit_kernels.hip are driven by.  Pure host code
// without a HIP type in it, so a stand-alone program can exercise it under a
// sanitizer (tests/audit_plan_check.cpp).  Host work is O(nreq) (times the
// tree height, and a sort for the overlap check): no per-node table is built,
// the kernels find a work item's node by arithmetic (audit_nodes.hpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/carbonado_hip_audit.h"
#include "audit_nodes.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace audit {

using rules::bao_content;
using rules::bao_len;
using rules::chunks;
using rules::ranges_overlap;
using rules::up;

constexpr uint64_t MAX_SLICE = 1ull << 53;  // index and count: start + len stays u64
constexpr uint64_t MAX_ITEMS = 1ull << 36;  // work items of one kind per call (a grid of < 2^31 workgroups)
constexpr uint64_t MAX_CONTENT = 1ull << 62;  // content bytes of a stream, where a call states them
constexpr uint64_t UNIT = 16;               // bytes per work item of the gathers

// One request, as the kernels read it (device scratch).
struct Req {
    uint64_t src;    // address of its stream, or of its proof (verify_proofs)
    uint64_t dst;    // address of its content range, or of its proof (extract)
    uint64_t hash;   // address of the 32 bytes its root is compared with
    uint64_t n;      // content bytes of the stream
    uint64_t N;      // chunks of the stream
    uint64_t first;  // selected chunks [first, last)
    uint64_t last;
    uint64_t olen;   // content bytes handed out
};
static_assert(sizeof(Req) == 64, "record layout");

// What a request (index, count <= MAX_SLICE) selects of n content bytes, in
// chunk units: start and len are multiples of 1024, so nothing can wrap.
struct Sel {
    uint64_t N, first, last, parents, proof_len, olen;
};
AUDIT_HD Sel select(uint64_t n, uint64_t index, uint64_t count) {
    Sel s;
    s.N = rules::chunks(n);
    s.first = umin(index, s.N - 1);
    s.last = umin(index + count, s.N);
    if (s.last < s.first + 1) s.last = s.first + 1;
    const uint64_t bytes = umin(n, s.last * 1024) - s.first * 1024;  // n = 0: the empty chunk
    s.parents = sel_parents(s.N, s.first, s.last);
    s.proof_len = 8 + 64 * s.parents + bytes;
    const uint64_t end = index + count >= s.N ? n : (index + count) * 1024;  // min(n, start + len)
    s.olen = index < s.N && index * 1024 < n ? end - index * 1024 : 0;
    return s;
}

inline int layout(const uint64_t *content_len, const uint64_t *index, const uint64_t *count, uint64_t nreq,
                  uint64_t align, uint64_t *proof_off, uint64_t *proof_len, uint64_t *content_off,
                  uint64_t *content_len_out, uint64_t *proof_total, uint64_t *content_total) {
    if (align == 0 || align % 16) return CHIP_ERR_INVALID_ARG;
    if (nreq && (!content_len || !index || !count)) return CHIP_ERR_INVALID_ARG;
    uint64_t p = 0, c = 0;
    for (uint64_t r = 0; r < nreq; ++r) {
        if (index[r] > MAX_SLICE || count[r] > MAX_SLICE || content_len[r] > MAX_CONTENT) return CHIP_ERR_INVALID_ARG;
        const Sel s = select(content_len[r], index[r], count[r]);
        if (proof_off) proof_off[r] = p;
        if (proof_len) proof_len[r] = s.proof_len;
        if (content_off) content_off[r] = c;
        if (content_len_out) content_len_out[r] = s.olen;
        p += up(s.proof_len, align);
        c += up(s.olen, align);
    }
    if (proof_total) *proof_total = p;
    if (content_total) *content_total = c;
    return CHIP_OK;
}

// scratch: [requests | parents prefix | chunks prefix | units prefix], each on a 256-B boundary
struct ScratchLayout {
    uint64_t reqs = 0, parents = 0, chunks = 0, units = 0, total = 0;
    explicit ScratchLayout(uint64_t nreq) {
        parents = up(nreq * sizeof(Req), 256);
        chunks = parents + up((nreq + 1) * 8, 256);
        units = chunks + up((nreq + 1) * 8, 256);
        total = units + up((nreq + 1) * 8, 256) + 16;
    }
};

inline uint64_t scratch_len(uint64_t /*nstreams*/, uint64_t nreq) { return ScratchLayout(nreq).total; }

// The table of one call, as uploaded, and the totals its launches need.
struct Plan {
    std::vector<uint8_t> table;
    uint64_t nreq = 0, total_parents = 0, total_chunks = 0, total_units = 0;
    ScratchLayout lay{0};
    Req *reqs() { return reinterpret_cast<Req *>(table.data()); }
    uint64_t *parents() { return reinterpret_cast<uint64_t *>(table.data() + lay.parents); }  // [nreq + 1]
    uint64_t *chunks() { return reinterpret_cast<uint64_t *>(table.data() + lay.chunks); }    // [nreq + 1]
    uint64_t *units() { return reinterpret_cast<uint64_t *>(table.data() + lay.units); }      // [nreq + 1]
};

// 16-B work items of a request's proof gather: the header, 4 per parent, 64 per chunk
inline uint64_t extract_units(uint64_t parents, uint64_t nchunks) { return 1 + 4 * parents + 64 * nchunks; }

// One request into the table; the prefix entries hold this request's counts
// until finish() turns them into prefix sums.
AUDIT_HD Req req_of(const Sel &s, uint64_t n, uint64_t src, uint64_t dst, uint64_t hash) {
    Req q;
    q.src = src; q.dst = dst; q.hash = hash; q.n = n;
    q.N = s.N; q.first = s.first; q.last = s.last; q.olen = s.olen;
    return q;
}

inline void put(Plan *p, uint64_t r, const Sel &s, uint64_t n, uint64_t src, uint64_t dst, uint64_t hash,
                uint64_t units) {
    p->reqs()[r] = req_of(s, n, src, dst, hash);
    p->parents()[r] = s.parents;
    p->chunks()[r] = s.last - s.first;
    p->units()[r] = units;
}

inline int finish(Plan *p) {
    uint64_t a = 0, b = 0, c = 0;
    for (uint64_t r = 0; r < p->nreq; ++r) {
        const uint64_t na = p->parents()[r], nb = p->chunks()[r], nc = p->units()[r];
        p->parents()[r] = a; p->chunks()[r] = b; p->units()[r] = c;
        a += na; b += nb; c += nc;
        if (a >= MAX_ITEMS || b >= MAX_ITEMS || c >= MAX_ITEMS) return CHIP_ERR_INVALID_ARG;
    }
    p->parents()[p->nreq] = a; p->chunks()[p->nreq] = b; p->units()[p->nreq] = c;
    p->total_parents = a; p->total_chunks = b; p->total_units = c;
    return CHIP_OK;
}

inline void start(Plan *p, uint64_t nreq) {
    p->nreq = nreq;
    p->lay = ScratchLayout(nreq);
    p->table.assign(p->lay.total - 16, 0);
}

// The content length of every stream of a call (BAO_TRUNCATED: no bao stream
// has that length) and its address check.
inline int stream_lengths(uintptr_t d_streams, const uint64_t *in_off, const uint64_t *in_len, uint64_t nstreams,
                          std::vector<uint64_t> *n, bool *truncated) {
    n->assign(nstreams, 0);
    for (uint64_t s = 0; s < nstreams; ++s) {
        if ((d_streams + in_off[s]) % 8) return CHIP_ERR_INVALID_ARG;
        if (!bao_content(in_len[s], &(*n)[s])) *truncated = true;
    }
    return CHIP_OK;
}

// Addresses are plain integers here (base + offset).  Every INVALID_ARG of a
// call is found before its first BAO_TRUNCATED is reported.
inline int plan_extract(uintptr_t d_streams, const uint64_t *in_off, const uint64_t *in_len, uint64_t nstreams,
                        const uint32_t *req_stream, const uint64_t *index, const uint64_t *count, uint64_t nreq,
                        uintptr_t d_proofs, const uint64_t *proof_off, const uint64_t *proof_len, Plan *p) {
    if (nreq == 0) return CHIP_OK;
    if (!d_streams || !in_off || !in_len || !req_stream || !index || !count || !d_proofs || !proof_off || !proof_len)
        return CHIP_ERR_INVALID_ARG;
    if (nreq >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> n;
    bool truncated = false;
    int st = stream_lengths(d_streams, in_off, in_len, nstreams, &n, &truncated);
    if (st != CHIP_OK) return st;
    start(p, nreq);
    for (uint64_t r = 0; r < nreq; ++r) {
        if (req_stream[r] >= nstreams || index[r] > MAX_SLICE || count[r] > MAX_SLICE) return CHIP_ERR_INVALID_ARG;
        if ((d_proofs + proof_off[r]) % 8) return CHIP_ERR_INVALID_ARG;
        const uint64_t s = req_stream[r];
        const Sel sel = select(n[s], index[r], count[r]);
        if (sel.proof_len != proof_len[r]) truncated = true;
        put(p, r, sel, n[s], d_streams + in_off[s], d_proofs + proof_off[r], 0, 0);
        p->units()[r] = extract_units(p->parents()[r], p->chunks()[r]);
    }
    if (ranges_overlap(proof_off, proof_len, nreq)) return CHIP_ERR_INVALID_ARG;
    st = finish(p);
    if (st != CHIP_OK) return st;
    return truncated ? CHIP_ERR_BAO_TRUNCATED : CHIP_OK;
}

// verify from the streams (d_src, src_off, src_len = d_streams, in_off, in_len
// per stream; one hash per stream) or from proofs (d_proofs, proof_off,
// proof_len per request; n = content_len[r]; one hash per request)
inline int plan_verify(bool proofs, uintptr_t d_src, const uint64_t *src_off, const uint64_t *src_len, uint64_t nstreams,
                       const uint32_t *req_stream, const uint64_t *content_len, uintptr_t d_hash,
                       const uint64_t *index, const uint64_t *count, uint64_t nreq, uintptr_t d_content,
                       const uint64_t *content_off, uint64_t *content_len_out, bool have_status_and_scratch, Plan *p) {
    if (nreq == 0) return CHIP_OK;
    if (!d_src || !src_off || !src_len || !index || !count || !content_off || !content_len_out ||
        !have_status_and_scratch || (proofs ? !content_len : !req_stream))
        return CHIP_ERR_INVALID_ARG;
    if (nreq >= (1ull << 31)) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> n;
    bool truncated = false;
    if (!proofs) {
        const int st = stream_lengths(d_src, src_off, src_len, nstreams, &n, &truncated);
        if (st != CHIP_OK) return st;
    }
    start(p, nreq);
    for (uint64_t r = 0; r < nreq; ++r) {
        if (index[r] > MAX_SLICE || count[r] > MAX_SLICE) return CHIP_ERR_INVALID_ARG;
        if (proofs ? content_len[r] > MAX_CONTENT : req_stream[r] >= nstreams) return CHIP_ERR_INVALID_ARG;
        const uint64_t s = proofs ? r : req_stream[r];
        const uint64_t nr = proofs ? content_len[r] : n[s];
        const Sel sel = select(nr, index[r], count[r]);
        const uint64_t src = d_src + src_off[s], dst = d_content + content_off[r];
        if (src % 8 || dst % 16) return CHIP_ERR_INVALID_ARG;
        if (sel.olen && !d_content) return CHIP_ERR_INVALID_ARG;
        if (proofs && sel.proof_len != src_len[r]) truncated = true;
        content_len_out[r] = sel.olen;
        put(p, r, sel, nr, src, dst, d_hash + 32 * s, (sel.olen + UNIT - 1) / UNIT);
    }
    if (ranges_overlap(content_off, content_len_out, nreq)) return CHIP_ERR_INVALID_ARG;
    const int st = finish(p);
    if (st != CHIP_OK) return st;
    if (truncated) return CHIP_ERR_BAO_TRUNCATED;
    return d_hash ? CHIP_OK : CHIP_ERR_HASH_DECODE;
}

}  // namespace audit
}  // namespace chip
