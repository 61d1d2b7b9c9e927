/*
 * carbonado_hip_audit.h — device-resident slice audits of libcarbonado_hip.so:
 * extract_slice / verify_slice (decoding.rs:116-149) for a batch of requests
 * over bao streams that stay in device memory.  Same library, same conventions
 * and status codes (chip_status) as carbonado_hip.h and carbonado_hip_ext.h,
 * which stay frozen at their versions; every name here is prefixed chipa_ and
 * versioned by CHIPA_ABI_VERSION.
 *
 * Terms.  A stream is a bao combined encoding (8-byte length header, then the
 * parent nodes and chunks in pre-order) of n content bytes.  A REQUEST r names
 * a slice of one stream: slice index[r] and count[r] in units of 1024 bytes,
 * that is start = index * 1024 and len = count * 1024 in u64 arithmetic (no
 * u16 wrap).  The chunks a request selects follow bao's rules: chunks
 * [first, last) with first = min(index, N - 1) and last = min(index + count, N),
 * at least one chunk (also for count == 0), N = max(1, ceil(n / 1024)); a start
 * at or past the end selects the last chunk.  Its PROOF is what
 * chip_bao_extract_slice returns: the stream's header, then, in pre-order, every
 * parent node whose subtree meets the selected chunks and the selected chunks;
 * chip_bao_slice_len(n, start, len) bytes.  Its CONTENT is content bytes
 * [start, min(n, start + len)), empty when start >= n.
 *
 * Who calls what.  The node holding the streams answers a batch of audit
 * requests with chipa_extract_slices_dev (proofs out, no hashing) or checks its
 * own holdings with chipa_verify_slices_dev (verdict and content straight from
 * the streams).  The auditor, holding only hashes and the proofs it was sent,
 * calls chipa_verify_proofs_dev.
 *
 * All three device calls: the arrays of per-request and per-stream numbers are
 * HOST arrays, read (or written) before the call returns; d_* are device
 * pointers.  The per-request table is uploaded into d_scratch
 * (chipa_audit_scratch_len bytes, 16-B aligned), and the kernels are enqueued
 * behind it on `stream` (a hipStream_t; NULL = the default stream) and not
 * synchronised; d_scratch belongs to the call until that work is done (calls on
 * one stream may share it).  The upload reads host memory at call time, so the
 * calls cannot be captured into a graph.  The number of kernel launches of a
 * call does not depend on nreq or nstreams.  Nothing is written outside the
 * stated output ranges, d_status[0, nreq) and the first chipa_audit_scratch_len
 * bytes of d_scratch.
 *
 * Decided on the host before anything is enqueued, in this order:
 * CHIP_ERR_INVALID_ARG for a NULL array or buffer with nreq > 0, a
 * req_stream[r] >= nstreams, an index or count above 2^53, a stream or proof
 * address (base + offset) that is not a multiple of 8, a content address that is
 * not a multiple of 16, two output ranges that overlap, or a call of 2^36 or
 * more selected nodes; CHIP_ERR_BAO_TRUNCATED for an in_len that is no bao
 * stream length or a proof_len that differs from chip_bao_slice_len;
 * CHIP_ERR_HASH_DECODE for a NULL d_hash; then CHIP_ERR_NO_DEVICE without a
 * usable device.  nreq == 0 is CHIP_OK and touches nothing.
 */
#ifndef CARBONADO_HIP_AUDIT_H
#define CARBONADO_HIP_AUDIT_H

#include "carbonado_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPA_API __attribute__((visibility("default")))
#else
#define CHIPA_API
#endif

#define CHIPA_ABI_VERSION 1

CHIPA_API int chipa_abi_version(void);

/* Host only, no device: the sizes of every request's proof and content and
 * where to put them.  content_len[r] = the content length n of request r's
 * stream.  proof_len[r] = chip_bao_slice_len(n, start, len) exactly;
 * content_len_out[r] = min(n, start + len) - start when start < n, else 0.
 * proof_off[r] / content_off[r] = offsets into one proof buffer and one content
 * buffer, each range starting on a multiple of `align` (a multiple of 16, not
 * 0); *proof_total / *content_total = the bytes those buffers need (each
 * length rounded up to `align`, nothing more).  Any of the six outputs may be
 * NULL. */
CHIPA_API int chipa_slice_layout(const uint64_t *content_len, const uint64_t *index, const uint64_t *count,
                                 uint64_t nreq, uint64_t align, uint64_t *proof_off, uint64_t *proof_len,
                                 uint64_t *content_off, uint64_t *content_len_out, uint64_t *proof_total,
                                 uint64_t *content_total);

/* Bytes of device scratch a call over nreq requests needs (any of the three
 * calls; nstreams is part of the signature for calls that may come to need
 * per-stream state and does not change the result today).  Host only. */
CHIPA_API uint64_t chipa_audit_scratch_len(uint64_t nstreams, uint64_t nreq);

/* The proof of every request, gathered on the device.  Stream s is
 * d_streams[in_off[s], in_off[s] + in_len[s]); its content length comes from
 * in_len[s].  Request r reads stream req_stream[r] and writes
 * d_proofs[proof_off[r], proof_off[r] + proof_len[r]), byte for byte what
 * chip_bao_extract_slice(stream, in_len, index[r], count[r] * 1024) returns.
 * proof_len[r] is an input and must be the exact length (chipa_slice_layout).
 * Pure selection: nothing is hashed and there is no per-request status; every
 * byte of each proof range is written and no other byte of d_proofs. */
CHIPA_API int chipa_extract_slices_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                                       uint64_t nstreams, const uint32_t *req_stream, const uint64_t *index,
                                       const uint64_t *count, uint64_t nreq, uint8_t *d_proofs,
                                       const uint64_t *proof_off, const uint64_t *proof_len, void *d_scratch,
                                       void *stream);

/* verify_slice of every request straight from the resident streams; d_hash +
 * 32 s = the expected root hash of stream s.  The nodes bao's slice decoder
 * would walk for the request (the selected chunks and every parent whose
 * subtree meets them) are re-hashed from their stored bytes and each is
 * compared with the chaining value stored in its own parent, the root with
 * the hash (a one-chunk stream is its own root); the stream's 8 header bytes
 * must equal its content length.  d_status[r] (device, uint32) = 0, or
 * CHIP_ERR_BAO_HASH_MISMATCH when any of those disagrees; damage elsewhere in
 * the stream, or in another stream, does not fail the request.
 * content_len[r] (host, written) = the request's content length;
 * d_content[content_off[r], content_off[r] + content_len[r]) holds the verified
 * content where d_status[r] is 0 and zeros otherwise, once the stream's work is
 * done: unverified bytes are never handed out. */
CHIPA_API int chipa_verify_slices_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                                      const uint8_t *d_hash, uint64_t nstreams, const uint32_t *req_stream,
                                      const uint64_t *index, const uint64_t *count, uint64_t nreq,
                                      uint8_t *d_content, const uint64_t *content_off, uint64_t *content_len,
                                      uint32_t *d_status, void *d_scratch, void *stream);

/* The auditor's side: the same verdict and content from the proofs alone.
 * Request r's proof is d_proofs[proof_off[r], proof_off[r] + proof_len[r]) as
 * chipa_extract_slices_dev (or chip_bao_extract_slice) wrote it,
 * content_len[r] the content length of the stream it was taken from (the
 * proof's header must say the same), d_hash + 32 r that stream's root hash:
 * one hash per REQUEST here.  The checks, d_status, content_len_out and
 * d_content are those of chipa_verify_slices_dev. */
CHIPA_API int chipa_verify_proofs_dev(const uint8_t *d_proofs, const uint64_t *proof_off, const uint64_t *proof_len,
                                      const uint64_t *content_len, const uint8_t *d_hash, const uint64_t *index,
                                      const uint64_t *count, uint64_t nreq, uint8_t *d_content,
                                      const uint64_t *content_off, uint64_t *content_len_out, uint32_t *d_status,
                                      void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_AUDIT_H */
