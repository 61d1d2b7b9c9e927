/*
 * carbonado_hip_read.h — ranged reads of libcarbonado_hip.so: byte ranges of
 * Zfec|Bao objects whose streams stay in device memory, served in one call and
 * rebuilt from other shards where the wanted shard's chunks are damaged (the
 * "degraded read" of an erasure code).  Same library, same conventions and
 * status codes (chip_status) as carbonado_hip.h, carbonado_hip_ext.h,
 * carbonado_hip_audit.h and carbonado_hip_repair.h, which stay frozen at their
 * versions; every name here is prefixed chipd_ and versioned by
 * CHIPD_ABI_VERSION.
 *
 * Terms.  STREAM s is d_streams[in_off[s], in_off[s] + in_len[s]), as in
 * carbonado_hip_repair.h: the bao combined encoding of the 8 zfec shards of one
 * object, chunk_len[s] = C bytes each, spc = C / 1024 chunks per shard; shard i
 * is chunks [i spc, (i + 1) spc) of the stream, shards 0..3 are the PRIMARIES.
 * Its OBJECT is the first n_obj = 4 C - padding[s] bytes of primaries 0..3 laid
 * end to end: object byte x is column x mod C of shard x / C.  REQUEST r is
 * (req_stream[r], start[r], len[r]) in object bytes at any alignment; its
 * CONTENT is object bytes [start, min(n_obj, start + len)), empty when start >=
 * n_obj or len == 0.  An empty request has status 0, used 0 and no work.  A
 * request is cut into at most four SEGMENTS, one per primary p it meets:
 * columns [c0, c1) of shard p.  The WINDOW of a segment is chunks
 * [w0, w1) = [c0 / 1024, ceil(c1 / 1024)) of a shard.  SLICE (segment, i) is
 * chunks [i spc + w0, i spc + w1) of the stream; it is AUTHENTIC exactly when
 * chipa_verify_slices_dev would give 0 for that chunk range: the chunks, every
 * parent whose subtree meets them, the root against d_hash + 32 s, and the
 * stream's header against its content length.  Damage outside the window does
 * not matter.
 *
 * Serving a segment.  Own slice (segment, p) authentic: the bytes are copied
 * from primary p's chunk slots.  Else, with at least 4 of the 8 slices
 * authentic: the first four authentic shares in ascending index (primaries
 * first, then secondaries: scrub's rule) are used, and the bytes are
 * sum_s coef[p][s] * share sel[s] at the same columns, coef = row p of the
 * inverse of those rows of zfec's 4-of-8 encoding matrix.  Fewer than 4: the
 * segment fails.
 *
 * Per-request results (device uint32 arrays, both set for every request):
 * d_status[r] = 0, or CHIP_ERR_ZFEC (7) when any of its segments fails, and
 * also when its stream's chunk_len does not fit (0, no multiple of 1024, not an
 * eighth of the stream's content) or padding > 4 C: such a request has content
 * length 0.  d_used[r] = 0 for a failed request, else the OR over its segments
 * of bit p (copied) or the bits of sel (rebuilt): 1 << p alone says the read
 * was direct.  Content is all or nothing per request:
 * d_content[content_off[r], content_off[r] + content_len[r]) holds the exact
 * bytes where the status is 0 and zeros otherwise; no other byte of d_content
 * is touched, nothing past scratch_len in d_scratch, and d_streams is never
 * written.
 *
 * What a rebuilt read guarantees.  Copied bytes are hashed against the root.
 * Rebuilt bytes are implied by four authentic shards; they are NOT themselves
 * hashed against the root.  That is the guarantee scrub's decode step has
 * before its re-encode check: four authentic shares of a stream that was never
 * a valid encoding decode to bytes no hash vouches for.  A caller who needs the
 * stronger guarantee scrubs the stream (chipr_scrub_ragged_dev) and reads the
 * result.
 *
 * Host arrays, the stream and the graph restriction are as in
 * carbonado_hip_audit.h: arrays of per-request and per-stream numbers are HOST
 * arrays read (content_len: written) before the call returns, d_* are device
 * pointers, `stream` is a hipStream_t (NULL = the default stream), and the
 * upload reads host memory at call time, so the call cannot be captured into a
 * graph.  d_scratch belongs to the call until its work is done.
 *
 * Work per call: one table upload (O(segments) bytes: one slice record and a
 * few words per segment, no per-node table), one memset, and at most 6 kernel
 * launches
 * whatever nreq, the sizes, the ranges and the damage (KA's parent and chunk
 * checks of the primary slices, the same two checks of the fallback slices,
 * the verdict per request, the read).  No synchronisation: the call returns
 * with everything enqueued on `stream`.  The 7 fallback slices of a segment
 * are hashed only when its own slice failed; the device decides, a fallback
 * work item whose segment's primary status is 0 returns before it loads a
 * node, so an intact read hashes one window per segment, not eight.
 *
 * Decided on the host before anything is enqueued, in this order:
 * CHIP_ERR_INVALID_ARG for a NULL array or buffer with nreq > 0 (d_content only
 * where some request has content), nreq >= 2^31, a req_stream[r] >= nstreams, a
 * start or len above 2^53, a stream address (base + offset) that is not a
 * multiple of 8, a content address that is not a multiple of 16, a d_scratch
 * that is not 16-B aligned, two content ranges that overlap, 2^36 or more work
 * items of one kind (2^31 slice requests or workgroups), or scratch_len <
 * chipd_read_scratch_len(nreq, segments of the call); CHIP_ERR_BAO_TRUNCATED
 * for an in_len that is no bao stream length; CHIP_ERR_HASH_DECODE for a NULL
 * d_hash; then CHIP_ERR_NO_DEVICE without a usable device.  nreq == 0 is
 * CHIP_OK and touches nothing.
 */
#ifndef CARBONADO_HIP_READ_H
#define CARBONADO_HIP_READ_H

#include "carbonado_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPD_API __attribute__((visibility("default")))
#else
#define CHIPD_API
#endif

#define CHIPD_ABI_VERSION 1

CHIPD_API int chipd_abi_version(void);

/* Host only, no device: where to put every request's content and how much a
 * call needs.  content_len[r] = the request's content length; content_off[r] =
 * its offset into one content buffer, every range starting on a multiple of
 * `align` (a multiple of 16, not 0); *content_total = the bytes that buffer
 * needs (each length rounded up to `align`, nothing more); *nseg = the
 * segments of the call, for chipd_read_scratch_len.  Any of the four outputs
 * may be NULL.  The stream lengths are not an input here, so a chunk_len that
 * is a multiple of 1024 counts as fitting; the read itself knows better, and a
 * request it refuses has length 0 and no segment there: the offsets and the
 * scratch length from here serve that call all the same. */
CHIPD_API int chipd_read_layout(const uint32_t *chunk_len, const uint32_t *padding, uint64_t nstreams,
                                const uint32_t *req_stream, const uint64_t *start, const uint64_t *len, uint64_t nreq,
                                uint64_t align, uint64_t *content_off, uint64_t *content_len, uint64_t *content_total,
                                uint64_t *nseg);

/* Bytes of device scratch a call of nreq requests in nseg segments needs; a
 * multiple of 16, growing with either.  Host only. */
CHIPD_API uint64_t chipd_read_scratch_len(uint64_t nreq, uint64_t nseg);

/* The content of every request, copied or rebuilt as above.  content_len[r]
 * (host, written) = the request's content length; content_off[r] as
 * chipd_read_layout gives it, or any other placement on multiples of 16 without
 * overlap.  d_status, d_used and the content are valid once the work enqueued
 * on `stream` is done. */
CHIPD_API int chipd_read_ranges_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                                    const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len,
                                    uint64_t nstreams, const uint32_t *req_stream, const uint64_t *start,
                                    const uint64_t *len, uint64_t nreq, uint8_t *d_content, const uint64_t *content_off,
                                    uint64_t *content_len, uint32_t *d_status, uint32_t *d_used, void *d_scratch,
                                    uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_READ_H */
