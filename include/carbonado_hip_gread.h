/*
 * carbonado_hip_gread.h — plaintext ranged reads of level-14 and level-15
 * objects planned on the device: chipf_read_ranges_dev of carbonado_hip_fread.h
 * for requests that live in device memory, over the stream table of
 * carbonado_hip_qread.h, a frame table that stays in device memory and, at 15,
 * the key table of carbonado_hip_kread.h.  Same library, same conventions and
 * status codes (chip_status) as the twelve older headers, which stay frozen at
 * their versions; every name here is prefixed chipg_ and versioned by
 * CHIPG_ABI_VERSION.
 *
 * Terms are those of carbonado_hip_fread.h (frame stream, frame index,
 * canonical, plain_len, index_status), carbonado_hip_qread.h (stream table,
 * info, request, capacity (nreq, max_len), content_stride, slot) and
 * carbonado_hip_kread.h (key table, killed).  What a read guarantees is what
 * carbonado_hip_fread.h states, unchanged: every frame handed out agreed with
 * the index entry it was read by and with its own CRC, the bytes behind it were
 * hashed against the stream's root as the vouch word says, and at 15 the GCM
 * tag is not checked.  What changes is who reads the requests and the indexes:
 *
 *   chipf_read_ranges_dev   the host walks every request, every stream and
 *       every index entry on every call, re-checks every index, builds and
 *       uploads three tables and, at 15, expands every stream's key.
 *   here   the streams are described once (chipq_stream_table_dev), their
 *       indexes once (chipg_frame_table_dev), at 15 their keys once
 *       (chipk_key_table_dev), and a read call takes the tables and three
 *       device arrays of requests.  Its host work is O(1); it uploads nothing,
 *       enqueues no memset and does not synchronise.
 *
 * The frame table.  chipg_frame_table_dev takes the HOST index arrays that
 * chipf_frame_index_dev or chipf_verify_index_dev proved (chunk_len, padding,
 * index_status, frame_off, idx_off, nframes, plain_len, one entry per stream;
 * index_status may be NULL: all 0) and makes, once, exactly the per-stream
 * checks chipf_read_ranges_dev makes on every call.  The table holds one
 * 32-byte record per stream (first entry, nframes, plain_len, index_status)
 * and, behind the records, the nframes + 1 entries of every stream whose
 * index_status is 0, compacted in stream order; a stream whose index_status is
 * not 0 has no entries and its index is not looked at.  It is one upload on
 * `stream`, no launch and no wait.  *finfo says what a read needs to know of
 * the table on the host: nstreams, nentries (the compacted entries),
 * max_frame (the largest off[f + 1] - off[f] among the streams whose
 * index_status is 0; 0: none) and the format.  On any error nothing is
 * uploaded and *finfo is zeroed.  The table stays valid as long as the streams
 * are not re-encoded; a scrub in place does not invalidate it.  It holds
 * nothing secret.
 *
 * The read.  chipg_read_ranges_dev works over the stream table and info of
 * chipq_stream_table_dev, a frame table and, where finfo->format is 15, a key
 * table, all made for the same streams in the same order.  Requests, capacity,
 * content_stride, the slot rule and "only [0, d_content_len[r]) of a slot is
 * written" are exactly those of carbonado_hip_qread.h; requests are in
 * PLAINTEXT bytes, as in carbonado_hip_fread.h: the content of request r is
 * plaintext [start, min(plain_len, start + len)) of its stream.
 *
 * Per-request results, decided on the device, in this order:
 *  1. d_status[r] = CHIP_ERR_INVALID_ARG (1), with content length 0, used 0 and
 *     vouch 0, for a stream index >= finfo->nstreams; a start or len above
 *     2^53; a content length (after clipping at the table's plain_len) above
 *     max_len; a frame record that contradicts finfo (its entries reach past
 *     nentries, or a touched frame is longer than max_frame); or anything the
 *     inner planned call refuses: a stream record that contradicts info, as in
 *     carbonado_hip_qread.h, or at 15 the cipher's limit of 2^36 - 32 bytes on
 *     one message, as in carbonado_hip_kread.h.
 *  2. Killed by the index: the stream's index_status is not 0.  d_status[r] is
 *     that word, d_content_len[r] the clipped length, zeros go over that range,
 *     d_used[r] = d_vouch[r] = 0; no hashing, keystream or decode work.
 *  3. At 15, killed by the key: the key table's key_status word is not 0.  The
 *     same with that word.
 *  4. Otherwise content bytes, content length, status (5, 7, 16 or 0), used and
 *     vouch are exactly what chipf_read_ranges_dev gives the same request
 *     placed at content_off[r] = r * content_stride with the same flags (0 or
 *     CHIPV_STRICT).  Content is all or nothing per request: zeros for every
 *     status other than 0.  An empty request (len 0, or start at or beyond
 *     plain_len) has status 0 and does no work.
 *
 * Work per call: kernel launches only, 15 at level 14 and 17 at level 15
 * whatever the requests: no upload, no memset, no allocation after the calling
 * thread's first call, no synchronisation.
 *   1 launch rewrites (one lane per request): it decides orders 1 and 2, takes
 *     f0 = start / 65536 and f1 = (end - 1) / 65536 and writes the frame-stream
 *     request (stream, off[f0], off[f1 + 1] - off[f0]) into the call's scratch;
 *     a refused request gets a stream index the inner planner refuses, a killed
 *     or empty one an empty len.
 *   The planned read of those requests into per-request staging slots in the
 *     scratch: at 14 chipq_read_ranges_vouched_dev's work (4 + 8 launches), at
 *     15 chipk_read_ranges_dev's (14 launches), whose "plaintext" is the frame
 *     stream.  Its capacity is (nreq, max_len') with max_len' = fcap *
 *     max_frame (1 where that is 0), fcap = (max_len + 65534) / 65536 + 1 being
 *     the frames a range of max_len bytes can touch; the staging stride is
 *     max_len' rounded up to 16.  Its content lengths live in the scratch; its
 *     status, used and vouch words are the caller's.
 *   1 block launch, one 64-lane workgroup per (request, k < fcap): frame
 *     f0 + k.  It leaves at once where f0 + k > f1 or d_status[r] is not 0;
 *     else it builds its work item in registers from the request and the frame
 *     table and does what the block decode of carbonado_hip_fread.h does:
 *     header against the index, block decode, CRC, the wanted bytes stored, a
 *     verdict word.  No item table, no search.
 *   1 finish launch, one workgroup per request: the verdict words combined,
 *     zeros and status 16 or the kill status where needed, and
 *     d_content_len[r] for every request.
 * Launch geometry depends on (info, finfo, nreq, max_len) alone and the
 * enqueued work reads no host memory: after one warm-up call a read can be
 * captured into a graph and replayed, any number of times, with the request
 * arrays rewritten in place.
 *
 * KEY MATERIAL.  As in carbonado_hip_kread.h: round keys live in the key table
 * only, a read puts nothing that depends on a key into its scratch (the
 * staging slots hold frame-stream bytes, which are data), so a read needs no
 * wipe; no load or store address and no branch depends on a key, a round key,
 * J0 or keystream.
 *
 * Decided on the host before anything is enqueued, in this order.
 * chipg_frame_table_dev: CHIP_ERR_INVALID_ARG for a NULL finfo; *finfo is
 * zeroed; then a format other than 14 and 15; nstreams == 0 is CHIP_OK, uploads
 * nothing and leaves finfo = {0, 0, 0, format}; then a NULL chunk_len, padding,
 * frame_off, idx_off, nframes, plain_len or d_ftable; nstreams >= 2^31; for
 * every stream whose index_status is 0, in stream order, an idx_off above 2^53,
 * nframes >= 2^31 or an index that does not fit (entries that do not ascend, a
 * last entry that is not the frame stream's length, a plain_len outside
 * (65536 (nframes - 1), 65536 nframes]), as chipf_read_ranges_dev; 2^30 or
 * more entries, a d_ftable that is not 16-B aligned, ftable_len <
 * chipg_frame_table_len(nstreams, entries of the streams whose status is 0);
 * then CHIP_ERR_NO_DEVICE.
 * chipg_read_ranges_dev: nreq == 0 is CHIP_OK and touches nothing; then
 * CHIP_ERR_INVALID_ARG for a NULL d_table, info, d_ftable, finfo, request
 * array, d_content, result array or d_scratch; a finfo->format other than 14
 * and 15; at 15 a NULL d_keytab; then everything
 * chipq_read_ranges_vouched_dev (at 14) or chipk_read_ranges_dev (at 15) lists,
 * in its order, for the capacity (nreq, max_len, content_stride); then max_len'
 * above 2^53, 2^31 or more block workgroups, more than 2^62 staging bytes, and
 * the same list for the inner capacity (nreq, max_len'); a d_ftable that is
 * not 16-B aligned; finfo->nstreams != info->nstreams; scratch_len <
 * chipg_read_scratch_len(info, finfo, nreq, max_len); then CHIP_ERR_NO_DEVICE.
 */
#ifndef CARBONADO_HIP_GREAD_H
#define CARBONADO_HIP_GREAD_H

#include "carbonado_hip_kread.h"
#include "carbonado_hip_fread.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPG_API __attribute__((visibility("default")))
#else
#define CHIPG_API
#endif

#define CHIPG_ABI_VERSION 1

typedef struct chipg_frame_info { /* host memory, 32 bytes */
    uint64_t nstreams;
    uint64_t nentries;  /* index entries in the table, all streams */
    uint64_t max_frame; /* the largest off[f+1] - off[f] among streams whose index_status is 0; 0: none */
    uint64_t format;    /* 14 or 15 */
} chipg_frame_info;

CHIPG_API int chipg_abi_version(void);

/* Bytes of device memory the frame table of nstreams streams with nentries
 * entries in all (nframes + 1 per stream, or any bound of it) needs; a multiple
 * of 16, growing with both, 0 for nstreams >= 2^31 or nentries >= 2^30.  Host
 * only. */
CHIPG_API uint64_t chipg_frame_table_len(uint64_t nstreams, uint64_t nentries);

/* The one description of the frame indexes of a set of resident streams.  All
 * arrays but d_ftable are host memory, one entry per stream, as
 * chipf_read_ranges_dev takes them; index_status may be NULL (all 0).
 * d_ftable: ftable_len bytes of device memory, 16-B aligned. */
CHIPG_API int chipg_frame_table_dev(uint8_t format, const uint32_t *chunk_len, const uint32_t *padding,
                                    const uint32_t *index_status, const uint64_t *frame_off, const uint64_t *idx_off,
                                    const uint64_t *nframes, const uint64_t *plain_len, uint64_t nstreams,
                                    void *d_ftable, uint64_t ftable_len, chipg_frame_info *finfo, void *stream);

/* Bytes of device scratch a read call of capacity (nreq, max_len) over the
 * tables `info` and `finfo` describe needs: the inner planned read's scratch,
 * the rewritten requests, a verdict word per (request, k) and nreq staging
 * slots; a multiple of 16, growing with nreq and max_len, 0 where the call
 * would refuse.  Host only. */
CHIPG_API uint64_t chipg_read_scratch_len(const chipq_table_info *info, const chipg_frame_info *finfo, uint64_t nreq,
                                          uint64_t max_len);

/* chipf_read_ranges_dev for requests in device memory.  d_status, d_used,
 * d_vouch, d_content_len and the content are valid once the work enqueued on
 * `stream` is done; d_scratch belongs to the call until then.  The tables are
 * read only.  d_keytab, keytab_len: looked at where finfo->format is 15. */
CHIPG_API int chipg_read_ranges_dev(const void *d_table, const chipq_table_info *info, const void *d_ftable,
                                    const chipg_frame_info *finfo, const void *d_keytab, uint64_t keytab_len,
                                    const uint32_t *d_req_stream, const uint64_t *d_start, const uint64_t *d_len,
                                    uint64_t nreq, uint64_t max_len, uint8_t *d_content, uint64_t content_stride,
                                    uint64_t *d_content_len, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch,
                                    uint32_t flags, void *d_scratch, uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_GREAD_H */
