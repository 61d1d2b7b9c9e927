/*
 * carbonado_hip_snap.h — the snappy framing format over device-resident
 * objects, the reference's Snappy stage (encoding.rs:16-28 `snap`,
 * decoding.rs:72-77), in libcarbonado_hip.so.  Same library, same conventions
 * and status codes (chip_status) as carbonado_hip.h, carbonado_hip_ext.h,
 * carbonado_hip_audit.h, carbonado_hip_repair.h, carbonado_hip_read.h,
 * carbonado_hip_vread.h and carbonado_hip_ecies.h, which stay frozen at their
 * versions; every name here is prefixed chips_ and versioned by
 * CHIPS_ABI_VERSION.  The device-resident entry points of those headers refuse
 * the Snappy bit exactly as before: nothing about them changes.
 *
 * The format is FrameEncoder's: the stream identifier, then one chunk per
 * 64 KiB block with the masked CRC-32C of the block and the block compressed,
 * or stored raw when compression saves less than 1/8.  The compressed bytes
 * are those of chip_snap_compress, bit for bit: the stream's bao hash is the
 * object's name, so "a valid snappy stream" would not be enough.  (Parity of
 * the host compressor with the snap crate itself is unpinned, as before;
 * nothing here changes the host compressor.)
 *
 * A call covers a ragged batch: object o has its own length, input offset and
 * output offset.  Host arrays have `count` entries and are read at call time
 * (so the calls cannot be captured into a graph); d_* pointers are device
 * memory; `stream` is a hipStream_t or NULL; d_scratch is 16-B aligned and
 * belongs to the call until its work is done.  The number of kernel launches
 * does not depend on count, the lengths or the data: 3 for a compress (blocks,
 * frame, gather), 4 for a decompress (walk, blocks, CRC, finish), each with
 * one table upload in front.  Host-decided errors come in the documented order
 * before anything is enqueued; count == 0 is CHIP_OK and touches nothing.
 *
 * Out of scope: formats 2 and 3 as one call (they are the raw calls here,
 * plus chipe_seal_ragged_dev / chipe_open_ragged_dev for 3).
 */
#ifndef CARBONADO_HIP_SNAP_H
#define CARBONADO_HIP_SNAP_H

#include "carbonado_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPS_API __attribute__((visibility("default")))
#else
#define CHIPS_API
#endif

#define CHIPS_ABI_VERSION 1

CHIPS_API int chips_abi_version(void);

/* Bytes of device scratch a compress / decompress call needs: a multiple of
 * 16.  0 for count == 0, a NULL array or lengths no call accepts.  Host only.
 * A compress keeps one private slot per 64 KiB block (about 1.17 x the input);
 * a decompress keeps 40 bytes per slot (below). */
CHIPS_API uint64_t chips_snap_scratch_len(const uint64_t *n, uint64_t count);
CHIPS_API uint64_t chips_unsnap_scratch_len(const uint64_t *in_len, const uint64_t *out_cap, uint64_t count);

/* encoding::snap of every object: the frame stream of object o (n[o] bytes at
 * d_in + in_off[o], 16-B aligned) to d_out + out_off[o], at any byte address,
 * capacity chip_snap_max_len(n[o]); its length to d_out_len[o] (device
 * uint64).  The bytes are those of chip_snap_compress; an empty object gives 0
 * bytes and no stream identifier.  Exactly d_out_len[o] bytes are written per
 * object and no other byte of d_out.  Does not synchronise.
 * Host-decided, in this order: CHIP_ERR_INVALID_ARG for a NULL in_off, n,
 * out_off, d_out_len or d_scratch; for count >= 2^31; for an object above
 * 2^40 bytes or 2^31 or more blocks in all; for a NULL d_in or d_out when some
 * object has bytes; for an offset above 2^53; for an input address of a
 * non-empty object that is not 16-B aligned; for a d_scratch that is not; for
 * two output ranges [out_off[o], out_off[o] + chip_snap_max_len(n[o])) that
 * overlap; for scratch_len below chips_snap_scratch_len.  Then
 * CHIP_ERR_NO_DEVICE. */
CHIPS_API int chips_snap_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                                    uint8_t *d_out, const uint64_t *out_off, uint64_t *d_out_len, void *d_scratch,
                                    uint64_t scratch_len, void *stream);

/* decoding::snap of every stream d_in + in_off[o], in_len[o] bytes, at any
 * byte address, into d_out + out_off[o] (16-B aligned), capacity out_cap[o].
 * d_status[o] (device uint32) and d_out_len[o] (device uint64) are what
 * chip_snap_decompress gives for the same bytes and capacity, in its order: a
 * framing error anywhere gives CHIP_ERR_SNAP; else a needed length above
 * out_cap[o] gives CHIP_ERR_BUFFER_TOO_SMALL with d_out_len[o] = the needed
 * length; else a block that does not decode, or whose CRC disagrees, gives
 * CHIP_ERR_SNAP.  Everything the host walk accepts is accepted: raw and
 * compressed chunks, skippable chunks 0x80-0xFE, a repeated stream
 * identifier, all four tag kinds, literal headers of 1-5 bytes.
 *
 * Damage: a framing error or a too-small buffer writes nothing into that
 * object's range (d_out_len[o] = 0 for the framing error); a block error gives
 * d_out_len[o] = 0 and zeros over [0, needed length): decompressed bytes of a
 * failed object never remain.  Other objects are unaffected.  A corrupt
 * stream ends in a status, never in a wait, and never writes outside its
 * object's range.
 *
 * Slots: object o may have ceil(out_cap[o] / 65536) + 1 data chunks.  Every
 * stream FrameEncoder or this library writes fits when out_cap[o] >= its
 * content (all their blocks but the last are full).  A valid stream with more
 * data chunks gets CHIP_ERR_UNSUPPORTED_FORMAT (11) and nothing written
 * (CHIP_ERR_SNAP and CHIP_ERR_BUFFER_TOO_SMALL take precedence over it): such
 * streams go through chip_snap_decompress.  Does not synchronise.
 * Host-decided, in this order: CHIP_ERR_INVALID_ARG for a NULL in_off, in_len,
 * out_off, out_cap, d_out_len, d_status or d_scratch; for count >= 2^31; for a
 * stream or a capacity above 2^40 bytes or 2^31 or more slots in all; for a
 * NULL d_in when some stream has bytes or a NULL d_out when some capacity is
 * non-zero; for an offset above 2^53; for an output address of a non-zero
 * capacity that is not 16-B aligned; for a d_scratch that is not; for two
 * ranges [out_off[o], out_off[o] + out_cap[o]) that overlap; for scratch_len
 * below chips_unsnap_scratch_len.  Then CHIP_ERR_NO_DEVICE. */
CHIPS_API int chips_unsnap_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len,
                                      uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                                      const uint64_t *out_cap, uint64_t *d_out_len, uint32_t *d_status,
                                      void *d_scratch, uint64_t scratch_len, void *stream);

/* ---- formats 6, 7, 10, 11, 14 and 15: Snappy with Bao and / or Zfec, with or
 * without Ecies, one call ---------------------------------------------------
 * `format` must have the Snappy bit and Bao, Zfec or both.  The encoded length
 * depends on the data, so the caller lays its rows out for the worst case:
 * chipx_ragged_layout at `format & 12` over chip_snap_max_len(n[o]), plus 97
 * with the Ecies bit; out_cap[o] is that worst-case encoded length.  Limit:
 * chip_snap_max_len(n[o]) (+ 97) <= 16 MiB.  Host only. */
CHIPS_API int chips_encode_layout(uint8_t format, const uint64_t *n, uint64_t count, uint64_t align,
                                  uint64_t stream_offset, uint64_t *out_off, uint64_t *out_cap, uint64_t *total);

/* Bytes of device scratch of the one-call forms: the frame streams (envelopes)
 * at 16-B aligned rows, the compressed lengths, the snap scratch and the
 * scratch of the ragged (Ecies) call behind them.  0 for a format, a NULL
 * array or lengths no call accepts.  Host only. */
CHIPS_API uint64_t chips_encode_scratch_len(uint8_t format, const uint64_t *n, uint64_t count);
CHIPS_API uint64_t chips_decode_scratch_len(uint8_t format, const uint64_t *in_len, const uint64_t *out_cap,
                                            uint64_t count);

/* encode() at `format` of every object: chips_snap_ragged_dev into rows of the
 * scratch; one gathered copy of the `count` compressed lengths back, for which
 * THE CALL WAITS ONCE because the layout of everything after depends on them;
 * then chipe_encode_ragged_dev at `format & 13` (Ecies bit) or
 * chipx_encode_ragged_dev at `format & 12` over the rows.  pubkey and inject
 * are used only with the Ecies bit.  Stream bytes, out_len (host), hash and
 * EncodeInfo (info may be NULL) are those of chip_encode at `format` with the
 * same injected values.  Exactly out_len[o] bytes are written per object.
 * Host-decided, in this order: CHIP_ERR_INVALID_ARG (the format; a NULL
 * in_off, n, out_off, out_len, d_out, d_hash or d_scratch, or pubkey with the
 * Ecies bit; a d_scratch off 16 B; count >= 2^31; an object whose worst case
 * is above 16 MiB; everything chips_snap_ragged_dev refuses; everything the
 * ragged encode refuses over the worst-case lengths, overlap included),
 * CHIP_ERR_ECIES for a receiver key that does not parse, CHIP_ERR_NO_DEVICE. */
CHIPS_API int chips_encode_ragged_dev(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len,
                                      const chip_ecies_inject *inject, const uint8_t *d_in, const uint64_t *in_off,
                                      const uint64_t *n, uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                                      uint64_t *out_len, uint8_t *d_hash, chip_encode_info *info, void *d_scratch,
                                      void *stream);

/* decode() at `format`: chipx_decode_ragged_dev at `format & 12`, or
 * chipe_decode_ragged_dev at `format & 13`, into rows of the scratch; then
 * chips_unsnap_ragged_dev into d_out + out_off[o] (16-B aligned, capacity
 * out_cap[o]).  An object that already has a bao, zfec or ecies status keeps
 * it: it is not decompressed, nothing of it is written and d_out_len[o] = 0.
 * Without the Ecies bit the call does not synchronise at all; with it, it has
 * the one wait the envelope open already has.  secret_key is used only with
 * the Ecies bit.
 * Host-decided, in this order: CHIP_ERR_INVALID_ARG (the format; a NULL d_in,
 * in_off, in_len, out_off, out_cap, d_out_len, d_status or d_scratch, or
 * secret_key with the Ecies bit; a d_scratch off 16 B; count >= 2^31), the
 * ragged decode's own errors (CHIP_ERR_INVALID_ARG, CHIP_ERR_BAO_TRUNCATED,
 * ...), CHIP_ERR_HASH_DECODE for a NULL d_hash with the Bao bit,
 * CHIP_ERR_INVALID_ARG for what chips_unsnap_ragged_dev refuses,
 * CHIP_ERR_ECIES for the secret key, CHIP_ERR_NO_DEVICE. */
CHIPS_API int chips_decode_ragged_dev(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                                      const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                                      const uint8_t *d_hash, const uint32_t *padding, uint8_t *d_out,
                                      const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len,
                                      uint32_t *d_status, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_SNAP_H */
