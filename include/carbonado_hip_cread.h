/*
 * carbonado_hip_cread.h — plaintext ranged reads of level-13 objects (Ecies |
 * Zfec | Bao) that stay in HBM, in libcarbonado_hip.so: the vouched ranged
 * reads of carbonado_hip_vread.h with the AES-256-GCM keystream of
 * carbonado_hip_ecies.h taken off the bytes they hand out.  Same library, same
 * conventions and status codes (chip_status) as carbonado_hip.h,
 * carbonado_hip_ext.h, carbonado_hip_audit.h, carbonado_hip_repair.h,
 * carbonado_hip_read.h, carbonado_hip_vread.h, carbonado_hip_ecies.h and
 * carbonado_hip_snap.h, which stay frozen at their versions; every name here is
 * prefixed chipc_ and versioned by CHIPC_ABI_VERSION.  The read and audit calls
 * of the older headers serve a level-13 stream as the level-12 stream of its
 * envelope exactly as before.
 *
 * Why a range can be read.  The envelope of an object is
 * eph_pub65 || nonce16 || tag16 || ciphertext, so plaintext byte x is envelope
 * byte x + 97; the cipher is CTR, so byte x needs keystream block x / 16 alone;
 * and the stream's bao root authenticates every ciphertext byte a vouched read
 * hands out.  Three layers, each usable alone: the keystream over ranges (1),
 * the keys of resident streams (2), the read (3).
 *
 * Host arrays are read at call time (so the calls cannot be captured into a
 * graph); d_* pointers are device memory; `stream` is a hipStream_t or NULL;
 * d_scratch belongs to the call until its work is done.  The number of kernel
 * launches does not depend on the batch.
 *
 * WHAT A READ GUARANTEES.  With status 0 and !(d_vouch[r] & CHIPV_UNVOUCHED)
 * (with CHIPV_STRICT: status 0 alone), the CIPHERTEXT behind every byte handed
 * out was hashed against the stream's root.  The GCM tag is NOT checked: that
 * needs the whole message.  Integrity therefore rests on the caller's trust in
 * the root hash, as it does for carbonado_hip_vread.h.  Nothing in a range
 * proves the KEY: a wrong secret key gives status 0 and bytes that are not the
 * plaintext.  A caller who needs the tag opens the object once with
 * chipe_decode_ragged_dev.
 *
 * Constant time, as in carbonado_hip_ecies.h: on the device no load or store
 * address and no branch depends on a key, a round key, H, J0 or keystream (AES
 * is the same bitsliced circuit in registers; a lane takes its neighbour's
 * keystream block through a lane shuffle, never through memory addressed by
 * data).  Positions, lengths, offsets, gate and status words do drive addresses
 * and branches.
 *
 * Key material.  The caller's keys and nonces, the round keys and J0 live in
 * the key region of a call's scratch, and the last operation calls (1) and (3)
 * enqueue overwrites that region with zeros (hipMemsetAsync).  The host staging
 * copy of the keys (pinned memory) is wiped by a host function enqueued behind
 * the upload, and the pageable table the call builds is wiped before the call
 * returns.  The keys chipc_stream_keys_dev writes to host memory are the
 * caller's to hold and wipe.
 */
#ifndef CARBONADO_HIP_CREAD_H
#define CARBONADO_HIP_CREAD_H

#include "carbonado_hip_ecies.h"
#include "carbonado_hip_vread.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPC_API __attribute__((visibility("default")))
#else
#define CHIPC_API
#endif

#define CHIPC_ABI_VERSION 1

CHIPC_API int chipc_abi_version(void);

/* ---- 1. the keystream over ranges ---------------------------------------------
 * Bytes of device scratch a call over nitems items under nkeys keys needs: a
 * multiple of 16, growing with either.  0 for nitems >= 2^31.  Host only. */
CHIPC_API uint64_t chipc_ctr_scratch_len(uint64_t nkeys, uint64_t nitems);

/* Item i XORs, in place, d_buf[buf_off[i], buf_off[i] + n[i]) with keystream
 * bytes [pos[i], pos[i] + n[i]) of AES-256-GCM under (keys[k], ivs[k]),
 * k = item_key[i]: keys 32 bytes and ivs 16 bytes per key (host), the cipher as
 * carbonado_hip_ecies.h states it (a 16-byte nonce, so J0 is the GHASH form;
 * real block b uses inc32^(b + 1)(J0), wrapping in the low 32 bits only).
 * pos[i] is any byte; d_buf + buf_off[i] is 16-B aligned.  It is XOR: the same
 * call encrypts and decrypts, and applied twice it is the identity.  d_gate:
 * NULL, or device uint32[nitems]: item i is skipped when d_gate[i] != 0 (read
 * once per work item, when the work runs).  No byte outside the item ranges is
 * written.  Does not synchronise.
 * Work: one table upload, 2 kernel launches (key setup: one wave per key that
 * some item uses: round keys, H and J0, none of the powers of H a tag needs;
 * ranges: one wave per 127 16-byte units of an item, each lane one bitsliced
 * evaluation of two keystream blocks) and one memset, whatever the items.
 * Host-decided, in this order: nitems == 0 is CHIP_OK and touches nothing.
 * CHIP_ERR_INVALID_ARG for a NULL keys, ivs, item_key, pos, n, buf_off or
 * d_scratch; for nitems >= 2^31; for an item_key[i] >= nkeys; for
 * pos[i] + n[i] > 2^36 - 32 or 2^31 or more work items in all; for an offset
 * above 2^53; for a NULL d_buf where some item has bytes; for a non-empty item
 * whose buffer address is not 16-B aligned; for a d_scratch that is not; for
 * two non-empty ranges that overlap; for scratch_len below
 * chipc_ctr_scratch_len(nkeys, nitems).  Then CHIP_ERR_NO_DEVICE. */
CHIPC_API int chipc_ctr_ranges_dev(const uint8_t *keys, const uint8_t *ivs, uint64_t nkeys, const uint32_t *item_key,
                                   const uint64_t *pos, const uint64_t *n, uint64_t nitems, uint8_t *d_buf,
                                   const uint64_t *buf_off, const uint32_t *d_gate, void *d_scratch,
                                   uint64_t scratch_len, void *stream);

/* ---- 2. the keys of resident streams ------------------------------------------
 * Bytes of device scratch chipc_stream_keys_dev needs for nstreams streams: a
 * multiple of 16, growing with it.  Host only. */
CHIPC_API uint64_t chipc_stream_keys_scratch_len(uint64_t nstreams);

/* The AES key and the nonce of every level-13 stream (the stream arguments of
 * chipv_read_ranges_dev): envelope bytes [0, 81), the ephemeral public key and
 * the nonce, are read by a vouched read under CHIPV_STRICT, so a key is only
 * ever derived from bytes hashed against the root (a header rebuilt from other
 * shards and vouched for is fine); one gathered copy brings them to the host
 * and THE CALL WAITS FOR IT ONCE, as chipe_open_ragged_dev does; the key
 * agreements run on the stage pool's threads.  Written, all host memory:
 * keys_out 32 bytes, ivs_out 16 bytes and key_status one uint32 per stream.
 * key_status[s]: 0; or the read's status, 5 or 7, for a header that could not
 * be served; or CHIP_ERR_ECIES (17) for a stream whose chunk_len and padding
 * give an object shorter than 97 bytes, or whose ephemeral key does not parse.
 * Where it is not 0 the key and the nonce are zeros.
 * Host-decided, in this order: nstreams == 0 is CHIP_OK.  CHIP_ERR_INVALID_ARG
 * (a NULL secret_key, keys_out, ivs_out, key_status or d_scratch; everything
 * chipv_read_ranges_dev refuses, in its order, with
 * chipc_stream_keys_scratch_len in the place of its scratch length),
 * CHIP_ERR_BAO_TRUNCATED, CHIP_ERR_HASH_DECODE, CHIP_ERR_ECIES for a secret key
 * that is not 32 bytes or not a scalar, CHIP_ERR_NO_DEVICE. */
CHIPC_API int chipc_stream_keys_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_streams,
                                    const uint64_t *in_off, const uint64_t *in_len, const uint8_t *d_hash,
                                    const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                                    uint8_t *keys_out, uint8_t *ivs_out, uint32_t *key_status, void *d_scratch,
                                    uint64_t scratch_len, void *stream);

/* ---- 3. the read ----------------------------------------------------------------
 * Requests are in PLAINTEXT bytes: the plaintext of stream s has
 * P = 4 chunk_len[s] - padding[s] - 97 bytes (0 where that is negative), and
 * the content of request r is plaintext [start[r], min(P, start[r] + len[r])).
 *
 * chipd_read_layout of the requests (req_stream[r], start[r] + 97, len[r]):
 * the same offsets, lengths, total and segment count.  Host only. */
CHIPC_API int chipc_read_layout(const uint32_t *chunk_len, const uint32_t *padding, uint64_t nstreams,
                                const uint32_t *req_stream, const uint64_t *start, const uint64_t *len, uint64_t nreq,
                                uint64_t align, uint64_t *content_off, uint64_t *content_len, uint64_t *content_total,
                                uint64_t *nseg);

/* Bytes of device scratch a read of nreq requests in nseg segments
 * (chipc_read_layout) over nstreams streams needs: chipv_read_scratch_len(nreq,
 * nseg) with the scratch of (1) behind it; a multiple of 16, growing with each.
 * Host only. */
CHIPC_API uint64_t chipc_read_scratch_len(uint64_t nreq, uint64_t nseg, uint64_t nstreams);

/* The plaintext of every request.  keys, ivs, key_status: host, one entry per
 * stream, as chipc_stream_keys_dev wrote them; key_status may be NULL (all 0).
 * The other arguments are those of chipv_read_ranges_dev, flags included.
 * The call (a) runs the vouched read of envelope bytes [97 + start[r], ...)
 * into the content ranges, with that call's plan, kernels and scratch layout,
 * (b) runs (1) over the same ranges in place with pos = start[r] and the gate
 * d_status, so that a failed request keeps its zeros, and (c) zeroes the key
 * region.  All of it is enqueued and nothing waited for: the at most 8
 * launches of the vouched read, the 2 of (1), two table uploads, two memsets.
 * d_used and d_vouch are the vouched read's.  d_status[r] is key_status of its
 * stream where that is non-zero: such a request gets zeros over its content
 * range, does no work in (a) or (b) and has d_used[r] = d_vouch[r] = 0;
 * otherwise it is the vouched read's status.  content_len[r] (host, written)
 * is the layout's whatever the status.  Content is all or nothing per request:
 * the exact plaintext for status 0, zeros otherwise, no other byte of
 * d_content touched, nothing past scratch_len in d_scratch, and d_streams is
 * never written.
 * Host-decided, in this order: nreq == 0 is CHIP_OK and touches nothing.
 * CHIP_ERR_INVALID_ARG for a NULL keys or ivs, then everything
 * chipv_read_ranges_dev lists, in its order, with chipc_read_scratch_len in the
 * place of its scratch length (a start above 2^53 - 97 is refused where that
 * call refuses one above 2^53; a plaintext range that ends above 2^36 - 32 is
 * refused with the scratch length): CHIP_ERR_INVALID_ARG,
 * CHIP_ERR_BAO_TRUNCATED, CHIP_ERR_HASH_DECODE, CHIP_ERR_NO_DEVICE. */
CHIPC_API int chipc_read_ranges_dev(const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status,
                                    const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                                    const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len,
                                    uint64_t nstreams, const uint32_t *req_stream, const uint64_t *start,
                                    const uint64_t *len, uint64_t nreq, uint8_t *d_content, const uint64_t *content_off,
                                    uint64_t *content_len, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch,
                                    uint32_t flags, void *d_scratch, uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_CREAD_H */
