/*
 * carbonado_hip_ext.h — extensions of libcarbonado_hip.so beyond the drop-in
 * boundary of carbonado_hip.h (which stays frozen at its ABI version): entry
 * points the reference crate has no counterpart for.  Same library, same
 * conventions and status codes (chip_status); every name here is prefixed
 * chipx_ and versioned by CHIPX_ABI_VERSION.
 *
 * Ragged device batches: encode() / decode() of `count` device-resident
 * objects of DIFFERENT lengths in one call, at the formats without host stages
 * (CHIP_FORMAT_BAO = 4, CHIP_FORMAT_ZFEC = 8, both = 12).  The number of kernel
 * launches of a call does not depend on `count`.  Object o has its own length,
 * input offset and output offset; its bytes, length, EncodeInfo, hash and
 * status are those chip_encode_batch_dev / chip_decode_batch_dev give for a
 * batch of that one object.
 *
 * Limits: an object is at most 16 MiB of input (decode: the encoding of such
 * an object); `count` and the call's total of 64-chunk groups are below 2^31.
 * Anything larger returns CHIP_ERR_INVALID_ARG before anything is enqueued:
 * larger objects go through the uniform entry points of carbonado_hip.h.
 */
#ifndef CARBONADO_HIP_EXT_H
#define CARBONADO_HIP_EXT_H

#include "carbonado_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPX_API __attribute__((visibility("default")))
#else
#define CHIPX_API
#endif

#define CHIPX_ABI_VERSION 1

CHIPX_API int chipx_abi_version(void);

/* Host only, no device: where a caller should put each object.  out_off[o] =
 * start of object o's output in one buffer, rows rounded up to `align` (a
 * multiple of 256), each Bao stream `stream_offset` bytes into its row (a
 * multiple of 8 below `align`; 56 = the fast layout of carbonado_hip.h; the
 * shards of a Zfec-only encoding start at the row's start whatever it is);
 * out_len[o] = its exact encoded length; *total = bytes the buffer needs. */
CHIPX_API int chipx_ragged_layout(uint8_t format, const uint64_t *n, uint64_t count, uint64_t align,
                                  uint64_t stream_offset, uint64_t *out_off, uint64_t *out_len, uint64_t *total);

/* Bytes of device scratch a ragged call over these objects needs: `len` = the
 * n array of an encode call (decode = 0) or the in_len array of a decode call
 * (decode = 1).  Host only. */
CHIPX_API uint64_t chipx_ragged_scratch_len(uint8_t format, const uint64_t *len, uint64_t count, int decode);

/* encode() of object o = d_in[in_off[o], in_off[o] + n[o]) into
 * d_out[out_off[o], out_off[o] + out_len[o]); its root hash to d_hash + 32 o
 * (zeros without the Bao bit), its EncodeInfo to info[o] (info may be NULL).
 *
 * in_off, n, out_off, out_len and info are HOST arrays of `count` entries,
 * read or written before the call returns; d_in, d_out, d_hash and d_scratch
 * (chipx_ragged_scratch_len bytes, 16-B aligned) are device pointers.  The
 * work, the upload of the per-object table into d_scratch included, is
 * enqueued on `stream` (a hipStream_t; NULL = the default stream, as the *_dev
 * entry points of carbonado_hip.h) and not synchronised; d_scratch belongs to
 * the call until that work is done (calls on one stream may share it).  The upload reads host memory at call time, so
 * the call cannot be captured into a graph.
 *
 * The call writes every byte of each object's output range and no other byte
 * of d_out, and nothing past chipx_ragged_scratch_len in d_scratch.
 *
 * Decided on the host before anything is enqueued: CHIP_ERR_INVALID_ARG for a
 * format with the Snappy or Ecies bit (or none of Bao / Zfec), an object over
 * 16 MiB, an input address (d_in + in_off[o]) that is not a multiple of 16, an
 * output address that is not a multiple of 8 (Bao streams) or 16 (Zfec-only
 * shards), or two objects whose output ranges overlap; then
 * CHIP_ERR_NO_DEVICE without a usable device.  count == 0 is CHIP_OK. */
CHIPX_API int chipx_encode_ragged_dev(uint8_t format, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n,
                                      uint64_t count, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                                      uint8_t *d_hash, chip_encode_info *info, void *d_scratch, void *stream);

/* decode() of the encoding d_in[in_off[o], in_off[o] + in_len[o]) with the
 * expected hash d_hash + 32 o (Bao bit) and padding[o] (Zfec bit) into
 * d_out[out_off[o], out_off[o] + out_len[o]).  d_status[o] (device, uint32) is
 * set for every object: 0, or CHIP_ERR_BAO_HASH_MISMATCH where any byte of
 * that object's stream or its hash disagrees; damage in one object changes
 * neither the status nor the bytes of another.  Host arrays, stream, scratch
 * and the graph restriction as above.
 *
 * Decided on the host before anything is enqueued: as above, with input
 * addresses multiples of 8 (Bao streams) or 16 (Zfec-only shards) and output
 * addresses multiples of 16; CHIP_ERR_BAO_TRUNCATED for an in_len that is no
 * bao stream length; CHIP_ERR_UNEVEN_ZFEC_CHUNKS where the bytes entering zfec
 * are not divisible by 8; CHIP_ERR_ZFEC for a padding above 4 shard lengths;
 * CHIP_ERR_HASH_DECODE for a NULL d_hash with the Bao bit. */
CHIPX_API int chipx_decode_ragged_dev(uint8_t format, const uint8_t *d_in, const uint64_t *in_off,
                                      const uint64_t *in_len, uint64_t count, const uint8_t *d_hash,
                                      const uint32_t *padding, uint8_t *d_out, const uint64_t *out_off,
                                      uint64_t *out_len, uint32_t *d_status, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_EXT_H */
