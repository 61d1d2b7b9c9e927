// paudit_device.hpp — one request of a device-planned slice audit into the
// record KA's checks read (include/carbonado_hip_paudit.h), and the arithmetic
// by which a work item of KB finds its request and slot.  Host/device code
// without a HIP type in it: paudit_kernels.hip runs it on the GPU, and the
// stand-alone tests/paudit_plan_check.cpp runs the same text on the host
// against audit::plan_verify / audit::plan_extract.  The selection, the parent
// count and the record are audit_plan.hpp's (audit::select, audit::req_of):
// nothing of them is stated here a second time.
//
// Every request of a call has the same capacity: P parent slots and max_count
// chunk slots.  A request that uses fewer leaves the rest without work; a work
// item compares its slot with the request's own counts and leaves.
#pragma once

#include "audit_plan.hpp"
#include "qread_device.hpp"

namespace chip {
namespace paudit {

using qread::StreamRec;  // the root table's records are the same, with src = 0

constexpr uint32_t NO_REQUEST = 0xFFFFFFFFu;

enum Kind : uint32_t { VERIFY = 0, EXTRACT = 1, PROOFS = 2 };

// What the host knows of a call: the table's info and the capacity.
struct Shape {
    uint64_t nstreams, max_chunks, max_count;
};

// One planned request: the record of KA's checks, its parent count and the
// words the caller reads.  A request without work has first = last and no
// parents; olen may still be stated (a proof of the wrong length).
struct Planned {
    audit::Req req;
    uint64_t parents;
    uint64_t proof_len;  // the exact length of its proof; 0 where refused or spare
    uint32_t status;
};

// Request (stream, index, count) of slot r.  content = the address of its
// content slot (VERIFY, PROOFS), proof = the address of its proof slot (EXTRACT,
// PROOFS), given_len = the proof bytes the caller states (PROOFS).
AUDIT_HD Planned plan_request(const StreamRec *recs, const Shape &sh, Kind kind, uint32_t stream, uint64_t index,
                              uint64_t count, uint64_t content, uint64_t proof, uint64_t given_len) {
    Planned p;
    p.req.src = 0; p.req.dst = 0; p.req.hash = 0; p.req.n = 0;
    p.req.N = 1; p.req.first = 0; p.req.last = 0; p.req.olen = 0;
    p.parents = 0; p.proof_len = 0; p.status = 0;
    if (stream == NO_REQUEST) return p;  // a spare slot
    p.status = CHIP_ERR_INVALID_ARG;
    if (stream >= sh.nstreams || index > audit::MAX_SLICE || count > audit::MAX_SLICE) return p;
    const StreamRec rec = recs[stream];
    if (rec.N > sh.max_chunks) return p;  // a table that is not the one info describes
    const audit::Sel s = audit::select(rec.n, index, count);
    if (s.last - s.first > sh.max_count) return p;
    p.status = 0;
    p.proof_len = s.proof_len;
    if (kind == PROOFS && given_len != s.proof_len) {  // no node of it is read; the content is zeros
        p.status = CHIP_ERR_BAO_TRUNCATED;
        p.req.olen = s.olen;
        p.req.dst = content;
        return p;
    }
    p.req = audit::req_of(s, rec.n, kind == PROOFS ? proof : rec.src, kind == EXTRACT ? proof : content,
                          kind == EXTRACT ? 0 : rec.hash);  // (audit::plan_extract's record has no hash either)
    p.parents = s.parents;
    return p;
}

// ---- work items ----------------------------------------------------------------
// Slot-major: item i of nreq x slots is slot i / nreq of request i % nreq, so the
// items of the first slots, which every request uses, fill whole workgroups and
// the workgroups of slots nobody uses leave together.  The gathers move `width`
// consecutive 16-B units per slot (4 of a parent, 64 of a chunk) on consecutive
// lanes, so a slot's bytes are one contiguous run of a wave's loads and stores.
struct Item {
    uint32_t r;
    uint64_t slot;
    uint32_t unit;  // within the slot: < width
};
AUDIT_HD Item item_of(uint64_t i, uint64_t nreq, uint32_t width) {
    Item it;
    it.unit = (uint32_t)(i % width);
    const uint64_t x = i / width;
    it.r = (uint32_t)(x % nreq);
    it.slot = x / nreq;
    return it;
}

// The proof gather's items: [nreq headers | nreq x P parents x 4 | nreq x max_count chunks x 64]
AUDIT_HD uint64_t extract_items(uint64_t nreq, uint64_t P, uint64_t max_count) {
    return nreq * (1 + 4 * P + 64 * max_count);
}

}  // namespace paudit
}  // namespace chip
