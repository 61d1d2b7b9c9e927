// kread_device.hpp — one plaintext request of a device-planned level-13 read
// (include/carbonado_hip_kread.h): what becomes of it, and the envelope request
// KQ's planner gets in its place.  Host/device code without a HIP type in it:
// kread_kernels.hip runs it one lane per request (the rewrite) and once per
// wave of a killed request (the keystream kernel), and the stand-alone
// tests/kread_plan_check.cpp runs the same text on the host against
// cread::shifted and the host call's decisions.  The range is read::range_of
// and the record checks are those of qread::plan_request: nothing of them is
// stated here a second time.
//
// Everything this text looks at is public: stream indices, positions, lengths,
// the stream records and the key_status words.  It touches no key.
#pragma once

#include "cread_device.hpp"
#include "qread_device.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace kread {

using rules::ENV_OVERHEAD;                     // eph_pub65 || nonce16 || tag16 in front of the ciphertext
constexpr uint32_t NO_STREAM = ~uint32_t(0);   // a stream index KQ's planner refuses: nstreams < 2^32

constexpr uint32_t REFUSED = 1;  // order 1 of the header: CHIP_ERR_INVALID_ARG, nothing read
constexpr uint32_t KILLED = 2;   // order 2: the stream's key_status word, zeros over the clipped range
constexpr uint32_t READ = 3;     // order 3: the vouched read of the envelope request, then the keystream

struct Decision {
    uint32_t order;
    uint32_t kill;     // KILLED: the key_status word
    uint64_t clen;     // KILLED: the clipped plaintext length
    uint32_t q_stream; // the envelope request KQ's planner gets
    uint64_t q_start, q_len;
};

// Request (stream, start, len) in plaintext bytes over the table sh describes.
AUDIT_HD Decision decide(const qread::StreamRec *recs, const uint32_t *key_status, const qread::Shape &sh,
                         uint32_t stream, uint64_t start, uint64_t len) {
    Decision d = {REFUSED, 0, 0, NO_STREAM, 0, 0};
    if (stream >= sh.nstreams || start > read::MAX_RANGE - ENV_OVERHEAD || len > read::MAX_RANGE) return d;
    const qread::StreamRec rec = recs[stream];
    if (rec.N > sh.max_chunks || (rec.C && rec.C < sh.min_shard)) return d;  // as qread::plan_request
    const read::Range rg = read::range_of(rec.C, rec.padding, start + ENV_OVERHEAD, len);
    const uint64_t clen = rg.end - rg.begin;
    if (clen > sh.max_len || rg.nseg > sh.S) return d;
    if (start > cread::MAX_END || clen > cread::MAX_END - start) return d;  // the keystream's limit on one message
    d.q_stream = stream;
    d.q_start = start + ENV_OVERHEAD;
    d.q_len = len;
    d.kill = key_status[stream];
    d.order = d.kill ? KILLED : READ;
    if (d.kill) {  // no hashing: the planner sees an empty request
        d.clen = clen;
        d.q_len = 0;
    }
    return d;
}

// ---- the bounded work mapping ------------------------------------------------------
// Work item w of a call of capacity (nreq, max_len) is (request, span) =
// (w / cap, w % cap), cap = cread::spans_of(max_len): a request's content
// length is max_len or less, so it has cap spans or fewer, and a work item
// whose span is past its request's leaves at once.
GCM_HD uint32_t span_cap(uint64_t max_len) { return uint32_t(cread::spans_of(max_len)); }

// The cread::Item of a request, built where the kernel builds it: no table.
GCM_HD cread::Item item_of_request(uint64_t r, uint64_t stride, uint64_t pos, uint64_t n, uint32_t key, uint32_t kill) {
    cread::Item it;
    it.buf_off = r * stride;
    it.pos = pos;
    it.n = n;
    it.work0 = 0;
    it.key = key;
    it.kill = kill;
    it.pad_ = 0;
    return it;
}

}  // namespace kread
}  // namespace chip
