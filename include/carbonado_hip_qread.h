/*
 * carbonado_hip_qread.h — ranged reads planned on the device: the ranged reads
 * of carbonado_hip_read.h and the vouched ranged reads of carbonado_hip_vread.h
 * for requests that live in device memory.  Same library, same conventions and
 * status codes (chip_status) as the ten older headers, which stay frozen at
 * their versions; every name here is prefixed chipq_ and versioned by
 * CHIPQ_ABI_VERSION.
 *
 * Terms are those of carbonado_hip_read.h and carbonado_hip_vread.h: stream,
 * object, request, content, segment, slice, authentic, the selection rule, the
 * classes of a rebuilt segment and the vouch word.  What a read guarantees is
 * unchanged.  What changes is who reads the requests:
 *
 *   chipd_read_ranges_dev / chipv_read_ranges_dev   the host walks every request
 *       and every stream of every call, builds a table of O(segments) bytes and
 *       uploads it; the upload reads host memory at call time.
 *   here   the streams of a set are described ONCE, by chipq_stream_table_dev,
 *       in a table that stays in device memory; a read call takes that table and
 *       three device arrays of requests, and a kernel plans them.  The host work
 *       of a read call is O(1): it reads no per-request and no per-stream array,
 *       uploads nothing, and does not synchronise.
 *
 * The stream table.  chipq_stream_table_dev makes, per stream, exactly the
 * checks chipd_read_ranges_dev makes per stream, in its order (below), and
 * uploads one record per stream (address, content bytes, chunks, shard length C,
 * padding, hash address; C = 0 where chunk_len does not fit the stream or
 * padding > 4 C) and behind them the 256-entry table mask of authentic slices ->
 * selected shares and inverse.  It fills *info (host) with the number of
 * streams, the largest chunk count and the smallest non-zero C among them; the
 * read calls size their grids from info alone.  The table stays valid while the
 * streams and their hashes stay where they are; scrubbing a stream in place
 * does not invalidate it.  The upload is enqueued on `stream`.
 *
 * Requests.  Request r is (d_req_stream[r], d_start[r], d_len[r]): a device
 * uint32 array and two device uint64 arrays of nreq entries, read by the GPU
 * only, after the work already enqueued on `stream`.  nreq and max_len are host
 * numbers, the CAPACITY of the call: a caller with fewer requests sets the spare
 * lengths to 0.  Request r's content goes to d_content + r * content_stride;
 * content_stride is a multiple of 16 and at least max_len rounded up to 16, and
 * d_content is 16-B aligned, so slots cannot overlap and there is no layout
 * call.  d_content_len[r] (device uint64, written) = the request's content
 * length.  Only bytes [0, d_content_len[r]) of a slot are written: the exact
 * bytes at status 0, zeros otherwise.  No other byte of d_content is touched,
 * nothing past scratch_len in d_scratch, and no stream is written.
 *
 * Per-request results, decided on the device (device uint32 arrays of nreq):
 * d_status[r] = CHIP_ERR_INVALID_ARG (1), with content length 0, used 0 and
 * vouch 0, for a stream index >= info->nstreams, a start or len above 2^53, a
 * content length (after clipping at the object's end) above max_len, or a
 * stream whose record contradicts info (more chunks than its largest, a
 * non-zero C below its smallest); then CHIP_ERR_ZFEC (7) for a stream whose C is
 * 0, as in carbonado_hip_read.h.  Every other request gets the content bytes,
 * status, used word and (vouched) vouch word that chipd_read_ranges_dev /
 * chipv_read_ranges_dev give the same request placed at content_off[r] =
 * r * content_stride.  An empty request has status 0 and no work.
 *
 * Work per call: kernel launches only, a fixed number of them: no upload and no
 * memset.  4 launches plan (one lane per request, which also zeroes the status
 * words the checks flag, where the host-planned calls enqueue a memset; then an
 * exclusive scan of the four work-item counts per segment slot in three
 * launches: per-workgroup scan, one workgroup over the workgroup sums, add; no
 * workgroup waits on another), then the 6 of chipd_read_ranges_dev or the 8 of
 * chipv_read_ranges_dev.  The host does not know the totals, so those launches
 * are sized by bounds from (info, nreq, max_len) and a work item past the true
 * total leaves at once.  Launch geometry depends on (info, nreq, max_len)
 * alone, nothing is allocated after the calling thread's first call and the
 * enqueued work reads no host memory: after one warm-up call a read call can
 * be captured into a graph and replayed, any number of times, with the request
 * arrays rewritten in place.
 *
 * Decided on the host before anything is enqueued, in this order.
 * chipq_stream_table_dev: CHIP_ERR_INVALID_ARG for a NULL info, a NULL array or
 * buffer with nstreams > 0, a NULL or not 16-B aligned d_table, nstreams >=
 * 2^32, a stream address (base + offset) that is not a multiple of 8, or
 * table_len < chipq_stream_table_len(nstreams); CHIP_ERR_BAO_TRUNCATED for an
 * in_len that is no bao stream length; CHIP_ERR_HASH_DECODE for a NULL d_hash;
 * then CHIP_ERR_NO_DEVICE.  On any error nothing is uploaded and *info (where
 * given) is zeroed.
 * The read calls: CHIP_ERR_INVALID_ARG for a NULL pointer with nreq > 0, nreq >=
 * 2^31, a max_len of 0 or above 2^53, a content_stride that is no multiple of
 * 16, below max_len rounded up to 16 or so large that a slot address wraps, a
 * d_content, d_table or d_scratch that is not 16-B aligned, a bit of flags other
 * than CHIPV_STRICT, bounds of 2^36 or more work items of one kind or 2^31
 * workgroups or segment slots, or scratch_len < chipq_read_scratch_len; then
 * CHIP_ERR_NO_DEVICE without a usable device.  nreq == 0 is CHIP_OK and touches
 * nothing.
 */
#ifndef CARBONADO_HIP_QREAD_H
#define CARBONADO_HIP_QREAD_H

#include "carbonado_hip_vread.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPQ_API __attribute__((visibility("default")))
#else
#define CHIPQ_API
#endif

#define CHIPQ_ABI_VERSION 1

/* What the read calls know of a stream table (host memory, 32 bytes). */
typedef struct chipq_table_info {
    uint64_t nstreams;
    uint64_t max_chunks; /* the largest chunk count among the streams */
    uint64_t min_shard;  /* the smallest non-zero shard length C; 0: no stream fits */
    uint64_t reserved;   /* 0 */
} chipq_table_info;

CHIPQ_API int chipq_abi_version(void);

/* Bytes of device memory the table of nstreams streams needs; a multiple of 16,
 * 0 for nstreams >= 2^32.  Host only. */
CHIPQ_API uint64_t chipq_stream_table_len(uint64_t nstreams);

/* The one upload of a set of resident streams.  The stream arguments are those
 * of chipd_read_ranges_dev, in its order (host arrays; d_streams and d_hash
 * device addresses).  d_table: table_len bytes of device memory, 16-B aligned.
 * *info is written on the host before the call returns. */
CHIPQ_API int chipq_stream_table_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                                     const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len,
                                     uint64_t nstreams, void *d_table, uint64_t table_len, chipq_table_info *info,
                                     void *stream);

/* Bytes of device scratch a read call of capacity (nreq, max_len) over the
 * table `info` describes needs (vouched != 0: the vouched call); a multiple of
 * 16, 0 where the call would refuse (nreq, max_len) or its bounds.  Host only. */
CHIPQ_API uint64_t chipq_read_scratch_len(const chipq_table_info *info, uint64_t nreq, uint64_t max_len,
                                          uint32_t vouched);

/* chipd_read_ranges_dev for requests in device memory.  d_status, d_used,
 * d_content_len and the content are valid once the work enqueued on `stream`
 * is done; d_scratch belongs to the call until then. */
CHIPQ_API int chipq_read_ranges_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                                    const uint64_t *d_start, const uint64_t *d_len, uint64_t nreq, uint64_t max_len,
                                    uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len,
                                    uint32_t *d_status, uint32_t *d_used, void *d_scratch, uint64_t scratch_len,
                                    void *stream);

/* chipv_read_ranges_dev for requests in device memory: d_vouch behind d_used
 * and flags (0 or CHIPV_STRICT) in front of d_scratch, as there. */
CHIPQ_API int chipq_read_ranges_vouched_dev(const void *d_table, const chipq_table_info *info,
                                            const uint32_t *d_req_stream, const uint64_t *d_start,
                                            const uint64_t *d_len, uint64_t nreq, uint64_t max_len, uint8_t *d_content,
                                            uint64_t content_stride, uint64_t *d_content_len, uint32_t *d_status,
                                            uint32_t *d_used, uint32_t *d_vouch, uint32_t flags, void *d_scratch,
                                            uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_QREAD_H */
