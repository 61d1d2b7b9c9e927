/*
 * carbonado_hip_paudit.h — slice audits planned on the device: the slice audits
 * of carbonado_hip_audit.h for requests, and on the auditor's side proofs, that
 * live in device memory.  Same library, same conventions and status codes
 * (chip_status) as the thirteen older headers, which stay frozen at their
 * versions; every name here is prefixed chipp_ and versioned by
 * CHIPP_ABI_VERSION.
 *
 * Terms are those of carbonado_hip_audit.h: stream, request (slice index and
 * count in units of 1024 bytes), the selected chunks [first, last), proof,
 * content.  What an audit checks and what it hands out is unchanged.  What
 * changes is who reads the requests:
 *
 *   chipa_extract_slices_dev / chipa_verify_slices_dev / chipa_verify_proofs_dev
 *       the host walks every request and every stream of every call, builds a
 *       table of 88 bytes per request and uploads it; the upload reads host
 *       memory at call time, so the calls cannot be captured into a graph.
 *   here   the streams of a set are described ONCE: on the holder's side by
 *       chipq_stream_table_dev (carbonado_hip_qread.h; an audit reads a record's
 *       address, content bytes, chunk count and hash address and ignores C and
 *       padding, so any bao stream serves and one table serves reads and audits
 *       alike), on the auditor's side, which holds no streams, by
 *       chipp_root_table_dev (content bytes, chunks and the address of the
 *       expected root per audited stream).  A call takes that table and three
 *       device arrays of requests, and a kernel plans them.  The host work of a
 *       call is O(1): it reads no per-request and no per-stream array, uploads
 *       nothing, and does not synchronise.
 *
 * Who calls what.  The node holding the streams answers a batch of challenges
 * with chipp_extract_slices_dev (proofs out, no hashing) or checks its own
 * holdings with chipp_verify_slices_dev.  The auditor, holding a root table and
 * the proofs it was sent, calls chipp_verify_proofs_dev.  The whole challenge /
 * response / check cycle is kernels only.
 *
 * Requests and slots.  Request r is (d_req_stream[r], d_index[r], d_count[r]):
 * a device uint32 array and two device uint64 arrays of nreq entries, read by
 * the GPU only, after the work already enqueued on `stream`.  nreq and
 * max_count >= 1 are host numbers, the CAPACITY of the call; max_count counts
 * the selected chunks of one request.  d_req_stream[r] == CHIPP_NO_REQUEST is a
 * spare slot: status 0, both lengths 0, no work.  Request r's content goes to
 * d_content + r * content_stride (content_stride a multiple of 16 and at least
 * 1024 * max_count) and d_content_len[r] (device uint64) is written; its proof
 * lives at d_proofs + r * proof_stride (proof_stride a multiple of 16 and at
 * least chipp_proof_bound(max_chunks, max_count)) and d_proof_len[r] (device
 * uint64) is written by extract and READ by verify_proofs.  Slots cannot
 * overlap, so there is no layout call.  Only bytes [0, len) of a slot are
 * written; no other byte of the output buffers is touched, nothing past
 * scratch_len in d_scratch, and no stream is written.
 *
 * Per-request status, decided on the device (d_status, device uint32 of nreq):
 * CHIP_ERR_INVALID_ARG (1), with lengths 0 and no work, for a stream index at or
 * above the table's count (other than CHIPP_NO_REQUEST), an index or count above
 * 2^53, a selection last - first above max_count (after clipping at the stream's
 * end, so a huge count on a short stream is fine), or a record with more chunks
 * than info->max_chunks.  In chipp_verify_proofs_dev a d_proof_len[r] that is
 * not the exact proof length gives CHIP_ERR_BAO_TRUNCATED (6): the content
 * length is still stated and the content is zeros.  Every other request gets
 * exactly what the chipa_* call gives the same request placed at content_off[r]
 * = r * content_stride or proof_off[r] = r * proof_stride: the same proof bytes,
 * the same status (0 or CHIP_ERR_BAO_HASH_MISMATCH), the same content bytes
 * (zeros where the status is not 0) and the same content length.  Extract has a
 * status array too (0 or 1), because the host can no longer refuse.
 *
 * Work per call: kernel launches only, a fixed number of them: 4 for
 * chipp_verify_slices_dev and chipp_verify_proofs_dev (plan, parent check,
 * chunk check, content gather / zero-fill), 2 for chipp_extract_slices_dev
 * (plan, proof gather).  No upload and no memset: the plan kernel, one lane per
 * request, writes every status word and length.  Every request has the same
 * capacity, so a work item finds its request and slot by arithmetic on its own
 * index: there is no prefix array, no scan and no search.  The grids are sized
 * from (info, nreq, max_count) alone, nothing is allocated after the calling
 * thread's first call and the enqueued work reads no host memory: after one
 * warm-up call a call can be captured into a graph and replayed, any number of
 * times, with the three request arrays (and for chipp_verify_proofs_dev the
 * proofs and d_proof_len) rewritten in place.
 *
 * Decided on the host before anything is enqueued, in this order.
 * chipp_root_table_dev: CHIP_ERR_INVALID_ARG for a NULL info, a NULL content_len
 * with nroots > 0, a NULL or not 16-B aligned d_table, nroots >= 2^32, a
 * content_len above 2^62, or table_len < chipp_root_table_len(nroots);
 * CHIP_ERR_HASH_DECODE for a NULL d_hash; then CHIP_ERR_NO_DEVICE.  On any error
 * nothing is uploaded and *info (where given) is zeroed.
 * The three calls: nreq == 0 is CHIP_OK and touches nothing; then
 * CHIP_ERR_INVALID_ARG for a NULL pointer, nreq >= 2^31, a max_count of 0 or
 * above 2^53, a stride that is no multiple of 16, below its minimum or so large
 * that a slot address wraps, a d_content, d_proofs, table or d_scratch that is
 * not 16-B aligned, bounds of 2^36 or more work items of one kind or 2^31
 * workgroups, or scratch_len < chipp_audit_scratch_len; then CHIP_ERR_NO_DEVICE
 * without a usable device.
 */
#ifndef CARBONADO_HIP_PAUDIT_H
#define CARBONADO_HIP_PAUDIT_H

#include "carbonado_hip_qread.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPP_API __attribute__((visibility("default")))
#else
#define CHIPP_API
#endif

#define CHIPP_ABI_VERSION 1

/* d_req_stream[r] of a spare slot */
#define CHIPP_NO_REQUEST 0xFFFFFFFFu

/* What chipp_verify_proofs_dev knows of a root table (host memory, 32 bytes). */
typedef struct chipp_root_info {
    uint64_t nroots;
    uint64_t max_chunks; /* the largest chunk count among the audited streams */
    uint64_t reserved[2]; /* 0 */
} chipp_root_info;

CHIPP_API int chipp_abi_version(void);

/* Bytes of device memory the table of nroots audited streams needs; a multiple
 * of 16, 0 for nroots >= 2^32.  Host only. */
CHIPP_API uint64_t chipp_root_table_len(uint64_t nroots);

/* The auditor's one upload: stream s has content_len[s] content bytes (host
 * array) and its expected root is the 32 bytes at d_hash + 32 s (device).
 * d_table: table_len bytes of device memory, 16-B aligned.  *info is written on
 * the host before the call returns; the upload is enqueued on `stream`. */
CHIPP_API int chipp_root_table_dev(const uint64_t *content_len, const uint8_t *d_hash, uint64_t nroots, void *d_table,
                                   uint64_t table_len, chipp_root_info *info, void *stream);

/* Bytes of device scratch a call of capacity (nreq, max_count) over a table
 * whose largest chunk count is info_max_chunks needs (any of the three calls);
 * a multiple of 16, 0 where the call would refuse (nreq, max_count) or its
 * bounds.  Host only. */
CHIPP_API uint64_t chipp_audit_scratch_len(uint64_t info_max_chunks, uint64_t nreq, uint64_t max_count);

/* The most bytes the proof of max_count selected chunks of a stream of
 * max_chunks chunks or fewer can have: 8 + 64 P + 1024 max_count, P the bound
 * of the selected parents; 0 for a max_count of 0 or above 2^53.  Host only. */
CHIPP_API uint64_t chipp_proof_bound(uint64_t max_chunks, uint64_t max_count);

/* chipa_verify_slices_dev for requests in device memory.  d_status,
 * d_content_len and the content are valid once the work enqueued on `stream`
 * is done; d_scratch belongs to the call until then. */
CHIPP_API int chipp_verify_slices_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                                      const uint64_t *d_index, const uint64_t *d_count, uint64_t nreq,
                                      uint64_t max_count, uint8_t *d_content, uint64_t content_stride,
                                      uint64_t *d_content_len, uint32_t *d_status, void *d_scratch,
                                      uint64_t scratch_len, void *stream);

/* chipa_extract_slices_dev for requests in device memory: d_proof_len[r] is
 * written, and d_status[r] is 0 or CHIP_ERR_INVALID_ARG. */
CHIPP_API int chipp_extract_slices_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                                       const uint64_t *d_index, const uint64_t *d_count, uint64_t nreq,
                                       uint64_t max_count, uint8_t *d_proofs, uint64_t proof_stride,
                                       uint64_t *d_proof_len, uint32_t *d_status, void *d_scratch,
                                       uint64_t scratch_len, void *stream);

/* chipa_verify_proofs_dev for requests and proofs in device memory: d_roots is
 * the table chipp_root_table_dev made, d_req_stream[r] names the audited stream
 * the proof in slot r was taken from, d_proof_len[r] the bytes that arrived. */
CHIPP_API int chipp_verify_proofs_dev(const void *d_roots, const chipp_root_info *root_info,
                                      const uint32_t *d_req_stream, const uint64_t *d_index, const uint64_t *d_count,
                                      uint64_t nreq, uint64_t max_count, const uint8_t *d_proofs,
                                      uint64_t proof_stride, const uint64_t *d_proof_len, uint8_t *d_content,
                                      uint64_t content_stride, uint64_t *d_content_len, uint32_t *d_status,
                                      void *d_scratch, uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_PAUDIT_H */
