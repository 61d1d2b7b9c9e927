/*
 * carbonado_hip_agree.h — the key agreement of the Ecies stage on the device:
 * secp256k1 scalar multiplication and HKDF-SHA256 as gfx950 kernels, and the
 * envelope calls of carbonado_hip_ecies.h rebuilt on them.  Same library, same
 * conventions and status codes (chip_status) as the fourteen older headers,
 * which stay frozen at their versions; every name here is prefixed chipy_ and
 * versioned by CHIPY_ABI_VERSION.
 *
 * What changes against carbonado_hip_ecies.h is who derives the AES keys:
 *
 *   chipe_seal_ragged_dev / chipe_encode_ragged_dev
 *       one key agreement per object (two scalar multiplications) runs on the
 *       host's stage pool before anything is enqueued;
 *   chipe_open_ragged_dev / chipe_decode_ragged_dev
 *       81 header bytes per envelope are copied back, THE CALL WAITS, the keys
 *       are derived on the pool and uploaded;
 *   here   the host uploads the scalars it must (the ephemeral secrets of a
 *       seal, 32 bytes each; the receiver's secret of an open, 32 bytes in
 *       all), and kernels do the rest: E = k G and k P of a seal by a
 *       fixed-base comb, one wave per object; sk R of an open by a fixed-window
 *       ladder, one lane per envelope; HKDF-SHA256(eph65 || shared65) in the
 *       same kernel, the AES key written straight into the key records the
 *       AES-GCM kernels read.  No key leaves device memory, nothing is copied
 *       back and no call here waits for the work it enqueues.  The host work of
 *       a call is the existing plan (offsets and lengths), the receiver's comb
 *       table (built once per receiver and thread, about 0.3 ms, 96 KiB
 *       uploaded per call) and, on a seal, the RNG.
 *
 * Where a call can still block.  (1) Every call uploads its scalars through
 * the calling thread's pinned staging copy, as the chipe_ and chipc_ calls do
 * their key tables (a host function behind the upload wipes the copy).  Before
 * a thread refills that copy it waits (hipEventSynchronize) until its PREVIOUS
 * key upload has run.  A second call on the same thread therefore blocks until
 * the first call's stream has reached that call's upload, which in an open, a
 * decode or the key table sits behind the header gather, the level-12 kernels
 * or the planned read.  It never waits for the kernels behind the upload.
 * (2) The first seal of a process builds the comb table of G and puts it into
 * device memory with hipMalloc and a synchronous copy on the null stream; the
 * table is kept per process, the library running one GPU per process.
 *
 * Host arrays have `count` entries and are read at call time (so the calls
 * cannot be captured into a graph); d_* pointers are device memory; `stream`
 * is a hipStream_t or NULL; d_scratch belongs to the call until its work is
 * done.
 *
 * Ephemeral public keys.  A 65-byte key is accepted in the form 0x04 || x || y
 * with x, y below p and on the curve, and in the hybrid forms 0x06 / 0x07 with
 * the same checks and the prefix's low bit equal to y's (OpenSSL's rule, which
 * the host decode follows); the HKDF input holds the 65 bytes exactly as the
 * envelope does, prefix included.  Every other key gives CHIP_ERR_ECIES (17)
 * for that object alone.
 *
 * Constant time.  The rule of carbonado_hip_ecies.h extends to the new
 * secrets: the ephemeral scalars, the receiver's secret scalar, every window
 * digit, every intermediate and shared point, the HKDF state and the derived
 * key.  On the device no load or store address and no branch depends on any of
 * them: tables are read whole under masks, selections are arithmetic, the
 * point formulas are complete (no special case for infinity, doubling or
 * inverses), the ladder and the inversion run a fixed number of steps.  Public
 * values do drive addresses and branches: the ephemeral PUBLIC keys and the
 * tables of their multiples, the receiver's public key and its table, lengths,
 * offsets, status words.  The two kernels keep every secret in registers: they
 * compile with a private segment of 0 bytes and use no LDS.
 *
 * Key material.  Host scalars reach the device through a pinned copy that a
 * host function enqueued behind the upload wipes; the pageable copy is wiped
 * before the call returns.  They live in the key region of the agreement
 * scratch, and the last operation every call enqueues overwrites that region
 * (and, in the envelope calls, the key region of the GCM scratch) with zeros.
 * The two raw calls leave AES keys in buffers the CALLER names: the caller
 * wipes them.
 *
 * Decided on the host before anything is enqueued, in this order.
 * chipy_seal_keys_dev: count == 0 is CHIP_OK and touches nothing;
 * CHIP_ERR_INVALID_ARG for a NULL pubkey, d_pub, d_keys or d_scratch, for
 * count >= 2^31, for pub_pitch below 65, key_pitch below 32 or either above
 * 2^32, for a d_scratch that is not 16-B aligned, for scratch_len below
 * chipy_keys_scratch_len(count); CHIP_ERR_ECIES for a receiver key that does
 * not parse; CHIP_ERR_ECIES for an injected secret that is 0, n or above n;
 * then CHIP_ERR_NO_DEVICE.
 * chipy_open_keys_dev: count == 0 is CHIP_OK; CHIP_ERR_INVALID_ARG for a NULL
 * secret_key, d_eph, d_keys, d_status or d_scratch and the cases above (with
 * eph_pitch for pub_pitch); CHIP_ERR_ECIES for sk_len != 32 or a secret that is
 * 0, n or above n; then CHIP_ERR_NO_DEVICE.
 * chipy_key_table_dev: a NULL info is CHIP_ERR_INVALID_ARG; info->nstreams == 0
 * is CHIP_OK; CHIP_ERR_INVALID_ARG for a NULL d_table, secret_key, d_keytab or
 * d_scratch, for 2^31 streams or more, for a d_table, d_keytab or d_scratch that
 * is not 16-B aligned, for keytab_len below chipk_key_table_len, for scratch_len
 * below chipy_key_table_scratch_len; CHIP_ERR_ECIES for the secret; then
 * CHIP_ERR_NO_DEVICE.
 * The envelope and one-call forms: the order of their chipe_ counterparts,
 * except that an injected secret that is no scalar is reported BEFORE
 * CHIP_ERR_NO_DEVICE (the host still decides it before anything is enqueued).
 */
#ifndef CARBONADO_HIP_AGREE_H
#define CARBONADO_HIP_AGREE_H

#include "carbonado_hip_ecies.h"
#include "carbonado_hip_kread.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPY_API __attribute__((visibility("default")))
#else
#define CHIPY_API
#endif

#define CHIPY_ABI_VERSION 1

CHIPY_API int chipy_abi_version(void);

/* Bytes of device scratch a key agreement over `count` objects needs (either
 * raw call): the receiver's comb table (96 KiB), 1536 bytes per object rounded
 * up to 64 objects for the tables of multiples of an open, 32 bytes per object
 * of scalars.  A multiple of 16; 0 for count == 0 or count >= 2^31.  Host
 * only.  One layout serves both directions, so each reserves what only the
 * other uses: a seal never touches the tables of multiples (25 MB of the
 * 25.8 MB at 16384 objects, about a third of chipy_envelope_scratch_len for
 * 64 KiB objects), an open and the key table never touch the 96 KiB comb
 * table.  Nothing reads or writes the unused part. */
CHIPY_API uint64_t chipy_keys_scratch_len(uint64_t count);

/* Per object o: the ephemeral public key E = k_o G as 0x04 || x || y to
 * d_pub + o pub_pitch (65 bytes) and the AES key HKDF(E65 || (k_o P)65) to
 * d_keys + o key_pitch (32 bytes).  pubkey: the receiver's key P, 33 or 65
 * bytes, parsed and checked once.  eph_sk: 32 bytes per object (host), or NULL
 * for secrets drawn from the library's RNG (rejection-sampled).  The two
 * outputs must not overlap; no other byte of them is written.  1 launch with
 * two uploads in front and one memset behind.  Does not synchronise. */
CHIPY_API int chipy_seal_keys_dev(const uint8_t *pubkey, uint64_t pubkey_len, const uint8_t *eph_sk, uint64_t count,
                                  uint8_t *d_pub, uint64_t pub_pitch, uint8_t *d_keys, uint64_t key_pitch,
                                  void *d_scratch, uint64_t scratch_len, void *stream);

/* Per object o: the AES key HKDF(R65 || (sk R)65) of the ephemeral key R at
 * d_eph + o eph_pitch (65 bytes, device) to d_keys + o key_pitch (32 bytes)
 * and d_status[o] (device uint32) = 0; or CHIP_ERR_ECIES and a key of zeros
 * for an R that does not parse, without disturbing the others.  1 launch with
 * one upload (the secret) in front and one memset behind.  Does not
 * synchronise. */
CHIPY_API int chipy_open_keys_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_eph, uint64_t eph_pitch,
                                  uint64_t count, uint8_t *d_keys, uint64_t key_pitch, uint32_t *d_status,
                                  void *d_scratch, uint64_t scratch_len, void *stream);

/* Bytes of device scratch chipy_seal_ragged_dev (n: the plaintext lengths) and
 * chipy_open_ragged_dev (n: the plaintext lengths, in_len - 97 or 0) need:
 * chipe_gcm_scratch_len(n, count) with chipy_keys_scratch_len(count) behind
 * it.  0 where either is.  Host only. */
CHIPY_API uint64_t chipy_envelope_scratch_len(const uint64_t *n, uint64_t count);

/* chipe_seal_ragged_dev with the key agreement on the device: the same
 * argument list, the same envelope bytes for the same injected values.  The
 * key kernel writes key records and header slots straight into the GCM
 * scratch; the setup, header scatter, span and finish launches follow.
 * d_scratch: chipy_envelope_scratch_len(n, count) bytes, 16-B aligned.  5
 * launches.  Does not synchronise. */
CHIPY_API int chipy_seal_ragged_dev(const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                                    const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                                    uint8_t *d_out, const uint64_t *out_off, void *d_scratch, void *stream);

/* chipe_open_ragged_dev with the key agreement on the device: the same
 * argument list, plaintext, out_len and status words.  The header gather runs,
 * the key kernel reads the header slots, writes the key records and marks an
 * envelope whose ephemeral key does not parse as refused, on the device; the
 * hash, verdict and gated CTR launches follow.  No copy back and no wait.
 * d_scratch: chipy_envelope_scratch_len(out_len, count) bytes.  6 launches. */
CHIPY_API int chipy_open_ragged_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                                    const uint64_t *in_off, const uint64_t *in_len, uint64_t count, uint8_t *d_out,
                                    const uint64_t *out_off, uint64_t *out_len, uint32_t *d_status, void *d_scratch,
                                    void *stream);

/* ---- formats 5, 9 and 13, one call: chipe_encode_ragged_dev and
 * chipe_decode_ragged_dev built on the two calls above.  Same argument lists,
 * stream bytes, hashes, EncodeInfo and status words for the same injected
 * values; the decode no longer blocks.  The scratch is the chipe_ forms' with
 * the agreement's scratch behind the GCM scratch. */
CHIPY_API uint64_t chipy_encode_scratch_len(uint8_t format, const uint64_t *n, uint64_t count);
CHIPY_API uint64_t chipy_decode_scratch_len(uint8_t format, const uint64_t *in_len, uint64_t count);

CHIPY_API int chipy_encode_ragged_dev(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len,
                                      const chip_ecies_inject *inject, const uint8_t *d_in, const uint64_t *in_off,
                                      const uint64_t *n, uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                                      uint64_t *out_len, uint8_t *d_hash, chip_encode_info *info, void *d_scratch,
                                      void *stream);

CHIPY_API int chipy_decode_ragged_dev(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                                      const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                                      const uint8_t *d_hash, const uint32_t *padding, uint8_t *d_out,
                                      const uint64_t *out_off, uint64_t *out_len, uint32_t *d_status, void *d_scratch,
                                      void *stream);

/* ---- the resident key table of level-13 streams without the host seeing a
 * header or a key: what chipc_stream_keys_dev followed by chipk_key_table_dev
 * produce (carbonado_hip_cread.h, carbonado_hip_kread.h), byte for byte, with no
 * copy back, no wait and no key in host memory.  d_table / info: the stream
 * table of chipq_stream_table_dev.  A kernel writes one request per stream
 * (envelope bytes [0, 81)); the device-planned strict vouched read fetches
 * them, so a key is only derived from bytes hashed against the stream's root;
 * the open key kernel writes key || nonce and the key_status word of every
 * stream into the table's staging part; the table's own key setup and finish
 * launches follow (the staging part is zeros again).  key_status: the read's
 * status (5, 7, ...); CHIP_ERR_ECIES (17) for an object too short to be an
 * envelope or an ephemeral key that does not parse.  The only upload is the
 * secret (32 bytes).  17 launches and two memsets.
 *
 * Bytes of device scratch; 0 for a NULL info, no streams or a table no read
 * accepts.  Host only. */
CHIPY_API uint64_t chipy_key_table_scratch_len(const chipq_table_info *info);

CHIPY_API int chipy_key_table_dev(const void *d_table, const chipq_table_info *info, const uint8_t *secret_key,
                                  uint64_t sk_len, void *d_keytab, uint64_t keytab_len, void *d_scratch,
                                  uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_AGREE_H */
