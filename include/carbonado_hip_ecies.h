/*
 * carbonado_hip_ecies.h — AES-256-GCM over device-resident messages, the data
 * half of the reference's Ecies stage (encoding.rs:30-36, decoding.rs:62-69),
 * in libcarbonado_hip.so.  Same library, same conventions and status codes
 * (chip_status) as carbonado_hip.h, carbonado_hip_ext.h, carbonado_hip_audit.h,
 * carbonado_hip_repair.h, carbonado_hip_read.h and carbonado_hip_vread.h, which
 * stay frozen at their versions; every name here is prefixed chipe_ and
 * versioned by CHIPE_ABI_VERSION.  The device-resident entry points of those
 * headers refuse the Ecies bit exactly as before (chip_encode_batch_dev,
 * chip_decode_batch_dev, chipx_encode_ragged_dev, chipx_decode_ragged_dev):
 * nothing about them changes.
 *
 * The cipher is AES-256-GCM as ecies 0.2.6 uses it: a 16-byte nonce, so
 * J0 = GHASH_H(IV || 0^64 || [128]_64) and not the 96-bit shortcut; no AAD;
 * counter blocks inc32(J0), inc32^2(J0), ... with the increment wrapping in the
 * low 32 bits only; tag = E_K(J0) ^ GHASH_H(C || [0]_64 [8 len]_64).
 *
 * A call covers a ragged batch: message o has its own key, nonce, length,
 * input offset and output offset.  Host arrays have `count` entries and are
 * read at call time (so the calls cannot be captured into a graph); d_*
 * pointers are device memory; `stream` is a hipStream_t or NULL; d_scratch
 * belongs to the call until its work is done.  The number of kernel launches
 * does not depend on count, the lengths or the verdicts: 3 for a seal (key
 * setup, CTR + GHASH, tags), 4 for an open (key setup, GHASH, verdicts, gated
 * CTR), each with one table upload in front and one memset behind.  A message
 * is spread over one wave per 8 KiB, so a 16 MiB message runs on 2048 waves.
 * Neither call synchronises: it returns with everything enqueued on `stream`.
 *
 * Constant time.  On the device no load or store address and no branch
 * depends on a key, a round key, H or its powers, a GHASH accumulator, the
 * keystream or the plaintext: AES is a bitsliced boolean circuit in registers
 * (no S-box or T-table in any memory), the GF(2^128) multiply is bit-serial
 * under masks (no Shoup table).  Ciphertext, lengths, offsets and verdict
 * words do drive addresses and branches.
 *
 * Open never shows unauthenticated plaintext: phase 1 computes the tag of the
 * ciphertext and compares all 16 bytes without early exit into a verdict word
 * per message; phase 2, the CTR pass, is gated on that word on the device.  A
 * message whose tag fails gets d_status[o] = CHIP_ERR_ECIES (17) and zeros
 * over its whole output range; the others get 0 and their plaintext.
 *
 * Key material.  The caller's keys and nonces, the round keys, the powers of
 * H, J0, E_K(J0) and the GHASH partial values live in the key region of the
 * call's scratch, and the last operation every call enqueues overwrites that
 * region with zeros (hipMemsetAsync).  The host staging copy of the keys
 * (pinned memory) is wiped with secure_wipe by a host function enqueued behind
 * the upload, and the pageable table the call builds is wiped before the call
 * returns.
 *
 * Decided on the host before anything is enqueued, in this order:
 * count == 0 is CHIP_OK and touches nothing.  CHIP_ERR_INVALID_ARG for a NULL
 * keys, ivs, in_off, n, out_off, d_tag, d_status (open) or d_scratch; for
 * count >= 2^31; for a message longer than 2^36 - 32 bytes or 2^31 or more
 * 8 KiB items in all; for a NULL d_in or d_out when some message has bytes;
 * for an offset above 2^53; for a plaintext address (d_in + in_off[o] of a
 * seal, d_out + out_off[o] of an open) of a non-empty message that is not
 * 16-B aligned; for a d_scratch that is not; for two non-empty output ranges
 * that overlap; for scratch_len below chipe_gcm_scratch_len.  Then
 * CHIP_ERR_NO_DEVICE.
 */
#ifndef CARBONADO_HIP_ECIES_H
#define CARBONADO_HIP_ECIES_H

#include "carbonado_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPE_API __attribute__((visibility("default")))
#else
#define CHIPE_API
#endif

#define CHIPE_ABI_VERSION 1

CHIPE_API int chipe_abi_version(void);

/* Bytes of device scratch a call over messages of these lengths needs: a
 * multiple of 16.  0 for count == 0, a NULL array or lengths no call accepts.
 * Host only. */
CHIPE_API uint64_t chipe_gcm_scratch_len(const uint64_t *n, uint64_t count);

/* Seal: ciphertext of message o (n[o] bytes of plaintext at d_in + in_off[o],
 * 16-B aligned) to d_out + out_off[o], at any byte address, and its 16-byte
 * tag to d_tag + 16 o.  keys: 32 bytes per message, ivs: 16 bytes per message
 * (host).  No byte outside the output ranges and the tags is written. */
CHIPE_API int chipe_gcm_seal_ragged_dev(const uint8_t *keys, const uint8_t *ivs, const uint8_t *d_in,
                                        const uint64_t *in_off, const uint64_t *n, uint64_t count, uint8_t *d_out,
                                        const uint64_t *out_off, uint8_t *d_tag, void *d_scratch,
                                        uint64_t scratch_len, void *stream);

/* Open: ciphertext of message o (n[o] bytes at d_in + in_off[o], any byte
 * address) and its tag at d_tag + 16 o; plaintext, or zeros, to
 * d_out + out_off[o] (16-B aligned); d_status[o] (device uint32) = 0 or
 * CHIP_ERR_ECIES.  d_in and d_tag are never written. */
CHIPE_API int chipe_gcm_open_ragged_dev(const uint8_t *keys, const uint8_t *ivs, const uint8_t *d_in,
                                        const uint64_t *in_off, const uint64_t *n, uint64_t count,
                                        const uint8_t *d_tag, uint8_t *d_out, const uint64_t *out_off,
                                        uint32_t *d_status, void *d_scratch, uint64_t scratch_len, void *stream);

/* encoding::ecies (encoding.rs:30-36 -> ecies::encrypt) of every object: the
 * envelope eph_pub65 || nonce16 || tag16 || ciphertext, n[o] + 97 bytes, to
 * d_out + out_off[o] (any byte address; 16-B aligned offsets put the
 * ciphertext at 1 mod 16, which the kernels take as it comes).  Plaintext o at
 * d_in + in_off[o], 16-B aligned.  The receiver key (33 or 65 bytes) is parsed
 * and checked once; one key agreement per object (two scalar multiplications)
 * runs on the stage pool's threads before anything is enqueued, and the host
 * time of a call is that; the nonces come from the library's RNG.  inject:
 * NULL, or `count` entries whose ephemeral_sk / nonce replace the random
 * values of object o (bit-exact tests).  d_scratch: at least
 * chipe_gcm_scratch_len(n, count) bytes, 16-B aligned.  4 launches.  Does not
 * synchronise.
 * Host-decided, in this order: CHIP_ERR_INVALID_ARG (a NULL pubkey, in_off, n,
 * out_off, d_out or d_scratch; count >= 2^31; an object above 2^36 - 32 bytes;
 * two envelopes that overlap; the cases of the raw seal), CHIP_ERR_ECIES for a
 * receiver key that does not parse, CHIP_ERR_NO_DEVICE, CHIP_ERR_ECIES for an
 * injected ephemeral secret that is not a scalar. */
CHIPE_API int chipe_seal_ragged_dev(const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                                    const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                                    uint8_t *d_out, const uint64_t *out_off, void *d_scratch, void *stream);

/* decoding::ecies (decoding.rs:62-69 -> ecies::decrypt) of every envelope
 * d_in + in_off[o], in_len[o] bytes, at any byte address: plaintext, or zeros,
 * to d_out + out_off[o] (16-B aligned); out_len[o] (host) = in_len[o] - 97, or
 * 0 for a shorter envelope; d_status[o] = 0 or CHIP_ERR_ECIES.  The 81 header
 * bytes of every envelope come back in one gathered copy and THE CALL WAITS
 * FOR IT ONCE, because the keys depend on them; the keys are derived on the
 * stage pool's threads; everything else is enqueued and not waited for.  An
 * envelope shorter than 97 bytes, or whose ephemeral key does not parse, gets
 * CHIP_ERR_ECIES in d_status (and zeros) without touching the others.
 * d_scratch: at least chipe_gcm_scratch_len(out_len, count) bytes.  1 + 4
 * launches.
 * Host-decided, in this order: CHIP_ERR_INVALID_ARG (a NULL secret_key, d_in,
 * in_off, in_len, out_off, out_len, d_status or d_scratch; count >= 2^31; the
 * cases of the raw open), CHIP_ERR_ECIES for a secret key that is not 32 bytes
 * or not a scalar, CHIP_ERR_NO_DEVICE. */
CHIPE_API int chipe_open_ragged_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                                    const uint64_t *in_off, const uint64_t *in_len, uint64_t count, uint8_t *d_out,
                                    const uint64_t *out_off, uint64_t *out_len, uint32_t *d_status, void *d_scratch,
                                    void *stream);

/* ---- formats 5, 9 and 13: Ecies with Bao and / or Zfec, one call ----------
 * The argument lists of chipx_encode_ragged_dev / chipx_decode_ragged_dev
 * (carbonado_hip_ext.h) with the key arguments above put in.  `format` must
 * have the Ecies bit, not the Snappy bit, and Bao, Zfec or both.  Limits as
 * in the ragged header, with n[o] + 97 <= 16 MiB.
 *
 * Bytes of device scratch: envelopes at 16-B aligned offsets, the GCM scratch
 * and the ragged call's scratch behind them.  0 for a format, a NULL array or
 * lengths no call accepts.  Host only. */
CHIPE_API uint64_t chipe_encode_scratch_len(uint8_t format, const uint64_t *n, uint64_t count);
CHIPE_API uint64_t chipe_decode_scratch_len(uint8_t format, const uint64_t *in_len, uint64_t count);

/* encode() at `format` of every object: chipe_seal_ragged_dev into envelopes
 * in the scratch, then chipx_encode_ragged_dev at `format & 12` over the
 * envelopes, as they are.  Stream bytes, hash and EncodeInfo (info may be
 * NULL) are those of chip_encode at `format` with the same injected values.
 * Does not synchronise.  Host-decided, in this order: CHIP_ERR_INVALID_ARG
 * (the format; a NULL pubkey, in_off, n, out_off, out_len, d_out, d_hash or
 * d_scratch; a d_scratch off 16 B; an object above 16 MiB - 97; everything
 * the ragged encode and the envelope seal refuse), CHIP_ERR_ECIES for a
 * receiver key that does not parse, CHIP_ERR_NO_DEVICE. */
CHIPE_API int chipe_encode_ragged_dev(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len,
                                      const chip_ecies_inject *inject, const uint8_t *d_in, const uint64_t *in_off,
                                      const uint64_t *n, uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                                      uint64_t *out_len, uint8_t *d_hash, chip_encode_info *info, void *d_scratch,
                                      void *stream);

/* decode() at `format`: chipx_decode_ragged_dev at `format & 12` into
 * envelopes in the scratch, then chipe_open_ragged_dev (which waits once for
 * the header bytes).  An object whose bao / zfec status is non-zero keeps that
 * status, as in chip_decode's order: it is not opened and its output is zeros.
 * out_len[o] (host) = the envelope's length - 97.  Host-decided, in this
 * order: the ragged decode's own errors (CHIP_ERR_INVALID_ARG,
 * CHIP_ERR_BAO_TRUNCATED, ...), CHIP_ERR_HASH_DECODE for a NULL d_hash with
 * the Bao bit, CHIP_ERR_INVALID_ARG for what the envelope open refuses,
 * CHIP_ERR_ECIES for the secret key, CHIP_ERR_NO_DEVICE. */
CHIPE_API int chipe_decode_ragged_dev(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                                      const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                                      const uint8_t *d_hash, const uint32_t *padding, uint8_t *d_out,
                                      const uint64_t *out_off, uint64_t *out_len, uint32_t *d_status, void *d_scratch,
                                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_ECIES_H */
