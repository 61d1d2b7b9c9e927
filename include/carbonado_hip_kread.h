/*
 * carbonado_hip_kread.h — plaintext ranged reads of level-13 objects planned on
 * the device: chipc_read_ranges_dev of carbonado_hip_cread.h for requests that
 * live in device memory, over the stream table of carbonado_hip_qread.h and a
 * key table that stays in device memory.  Same library, same conventions and
 * status codes (chip_status) as the eleven older headers, which stay frozen at
 * their versions; every name here is prefixed chipk_ and versioned by
 * CHIPK_ABI_VERSION.
 *
 * Terms are those of carbonado_hip_qread.h (stream table, info, request,
 * capacity (nreq, max_len), content_stride, slot) and carbonado_hip_cread.h
 * (envelope, plaintext, keystream, key_status, killed).  What a read guarantees
 * is what carbonado_hip_cread.h states, unchanged: with status 0 and
 * !(d_vouch[r] & CHIPV_UNVOUCHED) (with CHIPV_STRICT: status 0 alone) the
 * CIPHERTEXT behind every byte handed out was hashed against the stream's root;
 * the GCM tag is not checked and nothing in a range proves the key.  What
 * changes is who reads the requests and where the round keys live:
 *
 *   chipc_read_ranges_dev   the host walks every request and every stream,
 *       builds and uploads two tables, and expands every key some request uses
 *       on every call (one wave per key), then zeroes them.
 *   here   the streams are described once (chipq_stream_table_dev), their keys
 *       are expanded ONCE (chipk_key_table_dev), and a read call takes both
 *       tables and three device arrays of requests.  Its host work is O(1); it
 *       uploads nothing, enqueues no memset and does not synchronise.
 *
 * The key table.  chipk_key_table_dev does once what chipc_read_ranges_dev does
 * on every call.  keys (32 B per stream), ivs (16 B per stream) and key_status
 * (one uint32 per stream; NULL: all 0) are HOST arrays as chipc_stream_keys_dev
 * wrote them.  The table holds, per stream, one 512-byte record (the bitsliced
 * round keys and J0) and one key_status word, and behind them a staging part of
 * 48 bytes per stream.  The call uploads the words and the raw key || IV
 * records into the staging part (one upload, through a pinned copy that a host
 * function wipes behind it; the pageable copy is wiped before the call
 * returns), runs the key setup of carbonado_hip_cread.h over them, one wave per
 * stream, and then overwrites the staging part with zeros, all on `stream`: 2
 * launches.  A stream whose key_status is not 0 has zeros in its record and its
 * key is never uploaded.  The call waits for nothing (but the calling thread's
 * previous key upload) and is not meant to be captured into a graph.
 *
 * KEY MATERIAL, what changes.  In carbonado_hip_cread.h round keys and J0 live
 * in a call's scratch and are zeroed by the call.  Here they STAY in device
 * memory, in the buffer the caller owns, until the caller calls
 * chipk_key_table_wipe_dev, which overwrites the WHOLE table with zeros (a
 * memset; it enqueues only).  The raw keys and nonces are gone from the device
 * once chipk_key_table_dev's work is done.  A read call puts nothing that
 * depends on a key into its scratch, so a read needs no wipe.  The constant-
 * time rule of carbonado_hip_cread.h holds unchanged: on the device no load or
 * store address and no branch depends on a key, a round key, H, J0 or keystream.
 * Stream indices, positions, lengths, gate and status words (key_status among
 * them) are public and do drive addresses and branches.
 *
 * The read.  chipk_read_ranges_dev works over the stream table and info of
 * chipq_stream_table_dev and a key table made for the same streams in the same
 * order.  Requests, capacity, content_stride, the slot rule and "only
 * [0, d_content_len[r]) of a slot is written" are exactly those of
 * carbonado_hip_qread.h, with one difference: requests are in PLAINTEXT bytes.
 * The plaintext of stream s has P = n - 97 bytes (n: the object's, i.e. the
 * envelope's, bytes; P = 0 where that is negative), and the content of request
 * r is plaintext [start, min(P, start + len)).
 *
 * Per-request results, decided on the device, in this order:
 *  1. d_status[r] = CHIP_ERR_INVALID_ARG (1), with content length 0, used 0 and
 *     vouch 0, for a stream index >= info->nstreams; a start above 2^53 - 97 or
 *     a len above 2^53; a content length (after clipping at P) above max_len; a
 *     stream record that contradicts info, as in carbonado_hip_qread.h; or a
 *     plaintext range that ends above 2^36 - 32, the cipher's limit on one
 *     message (chipc_read_ranges_dev refuses the whole call for that; here the
 *     request is refused).
 *  2. Killed: the stream's key_status word is not 0.  d_status[r] is that
 *     word, d_content_len[r] the clipped plaintext length, zeros go over that
 *     range, d_used[r] = d_vouch[r] = 0, and the request does no hashing and no
 *     keystream work.
 *  3. Otherwise content bytes, content length, status, used and vouch are
 *     exactly what chipc_read_ranges_dev gives the same request placed at
 *     content_off[r] = r * content_stride with the same flags (0 or
 *     CHIPV_STRICT): CHIP_ERR_ZFEC (7) for a stream whose C is 0, 5 for a
 *     contradicted stream, the unvouched bit, and zeros for every status other
 *     than 0.
 *
 * Work per call: kernel launches only, 14 of them whatever the requests: no
 * upload, no memset, no allocation after the calling thread's first call, no
 * synchronisation.  1 launch rewrites (one lane per request: the decision of
 * orders 1 and 2 and the envelope request (stream, start + 97, len) into the
 * call's scratch; a refused request gets a stream index the planner refuses, a
 * killed one an empty len, so the planner does no work for either), then the 4
 * planning launches and the 8 of the vouched read of carbonado_hip_qread.h
 * over the rewritten requests, then 1 keystream launch: nreq * cap waves,
 * cap = the 127-unit spans of max_len bytes; wave w is request w / cap and span
 * w % cap, takes its key from the key table by the request's stream index, and
 * leaves at once where the span is past the request's content length or
 * d_status[r] is not 0; the waves of a killed request store its zeros and its
 * result words.  No item table, no search.  Launch geometry depends on (info,
 * nreq, max_len) alone and the enqueued work reads no host memory: after one
 * warm-up call a read can be captured into a graph and replayed, any number of
 * times, with the request arrays rewritten in place.
 *
 * Decided on the host before anything is enqueued, in this order.
 * chipk_key_table_dev: nstreams == 0 is CHIP_OK and touches nothing;
 * CHIP_ERR_INVALID_ARG for a NULL keys, ivs or d_keytab, a d_keytab that is not
 * 16-B aligned, nstreams >= 2^32, or keytab_len < chipk_key_table_len(nstreams);
 * then CHIP_ERR_NO_DEVICE.
 * chipk_key_table_wipe_dev: keytab_len == 0 is CHIP_OK; CHIP_ERR_INVALID_ARG
 * for a NULL d_keytab; then CHIP_ERR_NO_DEVICE.
 * chipk_read_ranges_dev: nreq == 0 is CHIP_OK and touches nothing; then
 * everything chipq_read_ranges_vouched_dev lists, in its order, where a NULL
 * d_keytab counts among the NULL pointers, a d_keytab that is not 16-B aligned
 * or keytab_len < chipk_key_table_len(info->nstreams) is reported where that
 * call reports a bad d_table, 2^31 or more keystream waves count among the
 * bounds, and chipk_read_scratch_len stands in the place of its scratch length:
 * CHIP_ERR_INVALID_ARG; then CHIP_ERR_NO_DEVICE.
 */
#ifndef CARBONADO_HIP_KREAD_H
#define CARBONADO_HIP_KREAD_H

#include "carbonado_hip_qread.h"
#include "carbonado_hip_cread.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPK_API __attribute__((visibility("default")))
#else
#define CHIPK_API
#endif

#define CHIPK_ABI_VERSION 1

CHIPK_API int chipk_abi_version(void);

/* Bytes of device memory the key table of nstreams streams needs; a multiple of
 * 16, growing with nstreams, 0 for nstreams >= 2^32.  Host only. */
CHIPK_API uint64_t chipk_key_table_len(uint64_t nstreams);

/* The one key setup of a set of resident level-13 streams.  keys, ivs,
 * key_status: host, one entry per stream, as chipc_stream_keys_dev wrote them;
 * key_status may be NULL (all 0).  d_keytab: keytab_len bytes of device memory,
 * 16-B aligned, the caller's until chipk_key_table_wipe_dev. */
CHIPK_API int chipk_key_table_dev(const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status,
                                  uint64_t nstreams, void *d_keytab, uint64_t keytab_len, void *stream);

/* Zeros over the whole table, enqueued on `stream` behind the reads that use it. */
CHIPK_API int chipk_key_table_wipe_dev(void *d_keytab, uint64_t keytab_len, void *stream);

/* Bytes of device scratch a read call of capacity (nreq, max_len) over the
 * table `info` describes needs: the vouched scratch of carbonado_hip_qread.h
 * with the rewritten requests behind it; a multiple of 16, growing with nreq
 * and max_len, 0 where the call would refuse (nreq, max_len) or its bounds.
 * Host only. */
CHIPK_API uint64_t chipk_read_scratch_len(const chipq_table_info *info, uint64_t nreq, uint64_t max_len);

/* chipc_read_ranges_dev for requests in device memory.  d_status, d_used,
 * d_vouch, d_content_len and the content are valid once the work enqueued on
 * `stream` is done; d_scratch belongs to the call until then.  d_keytab is read
 * only. */
CHIPK_API int chipk_read_ranges_dev(const void *d_table, const chipq_table_info *info, const void *d_keytab,
                                    uint64_t keytab_len, const uint32_t *d_req_stream, const uint64_t *d_start,
                                    const uint64_t *d_len, uint64_t nreq, uint64_t max_len, uint8_t *d_content,
                                    uint64_t content_stride, uint64_t *d_content_len, uint32_t *d_status,
                                    uint32_t *d_used, uint32_t *d_vouch, uint32_t flags, void *d_scratch,
                                    uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_KREAD_H */
