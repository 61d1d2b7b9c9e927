/*
 * carbonado_hip_repair.h — ragged scrub of libcarbonado_hip.so: scrub
 * (decoding.rs:151-212) of a batch of Bao|Zfec streams of different lengths
 * that stay in device memory, in one call.  Same library, same conventions and
 * status codes (chip_status) as carbonado_hip.h, carbonado_hip_ext.h and
 * carbonado_hip_audit.h, which stay frozen at their versions; every name here
 * is prefixed chipr_ and versioned by CHIPR_ABI_VERSION.
 *
 * Terms.  Stream o is d_in[in_off[o], in_off[o] + in_len[o]): the bao combined
 * encoding (8-byte length header, then parent nodes and chunks in pre-order) of
 * the 8 zfec shards of one object, chunk_len[o] bytes each (EncodeInfo's
 * chunk_len, a multiple of 1024), so its content is 8 * chunk_len[o] bytes.
 * SHARD i of the stream is its chunks [i * spc, (i + 1) * spc), spc =
 * chunk_len[o] / 1024; it is AUTHENTIC when that slice verifies against
 * d_hash + 32 o (decoding.rs:172-183: the chunks and every parent whose subtree
 * meets them, up to the root, and the stream's header).  The MASK of a stream
 * has bit i set when shard i is authentic; 0xFF is an intact stream.  A stream
 * whose 8 header bytes differ from its content length, or whose chunk_len[o]
 * is 0, no multiple of 1024 or not an eighth of its content, has mask 0.  A
 * stream with 4 to 7 authentic shards is REPAIRED: zfec-decoded from 4
 * authentic shards with their true share indices (primaries first, then
 * secondaries, in ascending order) to the 4 primaries, padding[o] bytes
 * dropped, and encode() at Zfec|Bao run again; the result is handed out only
 * when its hash equals d_hash + 32 o.
 *
 * Per-object result of chipr_scrub_ragged_dev (status[o], a HOST array, valid
 * when the call returns CHIP_OK; what chip_scrub_batch_dev reports for a batch
 * of that one stream):
 *   CHIP_ERR_UNNECESSARY_SCRUB (12)  all 8 shards authentic;
 *   CHIP_ERR_ZFEC (7)  fewer than 4 authentic shards (which includes mask 0
 *                      above), or padding[o] > 4 * chunk_len[o];
 *   CHIP_ERR_SCRUBBED_PADDING_MISMATCH (13) / _LENGTH_MISMATCH (14)  the
 *                      padding or stream length recomputed from
 *                      4 * chunk_len[o] - padding[o] bytes disagrees;
 *   CHIP_ERR_INVALID_SCRUBBED_HASH (15)  the re-encoded stream's hash differs;
 *   CHIP_OK (0)        repaired: d_out[out_off[o], out_off[o] + in_len[o]) holds
 *                      the stream, every byte of it written.
 * A per-object problem never fails the call or changes another object's
 * result.  An output range is written only where status[o] is 0; no other byte
 * of d_out is touched, nothing past scratch_len in d_scratch, and d_in is not
 * written, except that an object's output range may be exactly its input range
 * (d_out + out_off[o] == d_in + in_off[o]): the stream is repaired where it
 * lies.
 *
 * Arrays of per-stream numbers are HOST arrays read before the call returns;
 * d_* are device pointers.  The calls read host memory at call time and cannot
 * be captured into a graph.
 *
 * Work per call, whatever count, the mix of lengths and the damage:
 *   verdicts   the table of 8 slice requests per stream uploaded into
 *              d_scratch, one memset, then 3 launches (KA's parent and chunk
 *              checks, the fold of 8 status words into a mask).
 *              chipr_shard_masks_ragged_dev stops here, unsynchronised.
 *              chipr_scrub_ragged_dev copies the masks back: 1 synchronisation;
 *   repair     the streams to repair, in object order, packed into as many
 *              PASSES as the given scratch requires (scratch of
 *              chipr_scrub_ragged_scratch_len(.., nrepair = count): one pass).
 *              Each pass: 2 table uploads, 6 launches (repair_decode_kernel,
 *              KR's parity, group and top kernels, the hash compare, the
 *              gather of the matching rows to their output ranges), one copy
 *              of the verdicts back, 1 synchronisation.  Results do not depend
 *              on the number of passes.
 *
 * Decided on the host before anything is enqueued, in this order:
 * CHIP_ERR_INVALID_ARG for a NULL array or buffer with count > 0, count >=
 * 2^31, a stream or output address (base + offset) that is not a multiple of 8,
 * a d_scratch that is not 16-B aligned, two output ranges that overlap or an
 * output range that overlaps any input range other than by being exactly its
 * own, a stream whose content exceeds 32 MiB (the encoding of a 16 MiB object),
 * or scratch_len < chipr_scrub_ragged_scratch_len(in_len, count, 1) (both
 * calls, so one scratch serves them); CHIP_ERR_BAO_TRUNCATED for an in_len
 * that is no bao stream length; CHIP_ERR_HASH_DECODE for a NULL d_hash; then
 * CHIP_ERR_NO_DEVICE without a usable device.  count == 0 is CHIP_OK and
 * touches nothing.  (The output-side checks are chipr_scrub_ragged_dev's.)
 */
#ifndef CARBONADO_HIP_REPAIR_H
#define CARBONADO_HIP_REPAIR_H

#include "carbonado_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPR_API __attribute__((visibility("default")))
#else
#define CHIPR_API
#endif

#define CHIPR_ABI_VERSION 1

CHIPR_API int chipr_abi_version(void);

/* Host only.  Scratch for a call over these streams that can repair any
 * `nrepair` of them in one pass (nrepair clamped to [1, count]); a multiple of
 * 16.  Lengths a call would reject count as empty. */
CHIPR_API uint64_t chipr_scrub_ragged_scratch_len(const uint64_t *in_len, uint64_t count, uint64_t nrepair);

/* Verdicts only, enqueued on `stream` (a hipStream_t; NULL = the default
 * stream), not synchronised: d_masks[o] (device, uint32) = the mask of stream
 * o.  Writes d_masks[0, count) and d_scratch (which belongs to the call until
 * that work is done) and nothing else. */
CHIPR_API int chipr_shard_masks_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len,
                                           uint64_t count, const uint8_t *d_hash, const uint32_t *chunk_len,
                                           uint32_t *d_masks, void *d_scratch, uint64_t scratch_len, void *stream);

/* scrub (decoding.rs:151-212) of every stream; synchronous; status is a HOST array. */
CHIPR_API int chipr_scrub_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len,
                                     uint64_t count, const uint8_t *d_hash, const uint32_t *padding,
                                     const uint32_t *chunk_len, uint8_t *d_out, const uint64_t *out_off,
                                     int32_t *status, void *d_scratch, uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_REPAIR_H */
