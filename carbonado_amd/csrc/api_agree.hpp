// api_agree.hpp — what api_agree.cpp and api_ecies.cpp share: the envelope
// calls of api_ecies.cpp with the place the keys come from as a parameter
// (the host's stage pool, as the chipe_* calls; the KY kernels, as the chipy_*
// calls), and the pieces of a device key agreement that api_agree.cpp enqueues
// for them and for its own raw calls.
#pragma once

#include <functional>
#include <vector>

#include "agree_kernels.hpp"
#include "api_common.hpp"
#include "carbonado_hip_agree.h"

namespace chip {
namespace api {

enum class KeySource { Host, Device };

// ---- api_ecies.cpp: chipe_* (Host) and chipy_* (Device) are these -------------------
// Device: d_scratch holds the GCM scratch and, behind it, the agreement's
// (chipy_envelope_scratch_len); an injected secret that is no scalar is
// reported before CHIP_ERR_NO_DEVICE; nothing is copied back or waited for.
int ecies_seal_env(KeySource src, const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                   const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count, uint8_t *d_out,
                   const uint64_t *out_off, void *d_scratch, void *stream);
int ecies_open_env(KeySource src, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in, const uint64_t *in_off,
                   const uint64_t *in_len, uint64_t count, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                   uint32_t *d_status, void *d_scratch, void *stream, bool keep_status, bool check_only);
uint64_t ecies_encode_scratch_len(KeySource src, uint8_t format, const uint64_t *n, uint64_t count);
uint64_t ecies_decode_scratch_len(KeySource src, uint8_t format, const uint64_t *in_len, uint64_t count);
int ecies_encode_env(KeySource src, uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len,
                     const chip_ecies_inject *inject, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n,
                     uint64_t count, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, uint8_t *d_hash,
                     chip_encode_info *info, void *d_scratch, void *stream);
int ecies_decode_env(KeySource src, uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                     const uint64_t *in_off, const uint64_t *in_len, uint64_t count, const uint8_t *d_hash,
                     const uint32_t *padding, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                     uint32_t *d_status, void *d_scratch, void *stream);

// ---- api_agree.cpp: the pieces of a device key agreement ------------------------------
// n bytes from the library's RNG in as few calls as it takes; false where it fails
bool agree_rand(uint8_t *p, size_t n);

// The scalars of `count` objects as the kernels read them (32 bytes each):
// injected(o), or NULL for one drawn from the library's RNG (rejection-sampled).
// CHIP_ERR_ECIES for an injected one that is no scalar; then *words is wiped.
int agree_draw(uint64_t count, const std::function<const uint8_t *(uint64_t)> &injected, std::vector<uint8_t> *words);

// Receiver table and scalars into the agreement scratch `ascr` (the scalars
// through the pinned-and-wiped path; `words` is wiped), then the seal kernel:
// object o's public key to pub + o pub_pitch, its AES key to keys + o key_pitch.
hipError_t agree_seal_enqueue(Ctx *c, const uint8_t peer[65], std::vector<uint8_t> &words, uint64_t count, uint8_t *ascr,
                              uint8_t *pub, uint64_t pub_pitch, uint8_t *keys, uint64_t key_pitch, hipStream_t s);

// The receiver's secret (32 bytes, a scalar) into the agreement scratch `ascr`
// (sized for L.count objects), then the open kernel.  The caller fills what the
// kernel reads and writes (agree_kernels.hpp: the ephemeral keys and their
// pitch, the key slots, and whichever of status, refused, copy_iv, gate and
// shorter it wants); sk and vtab are set here.
hipError_t agree_open_enqueue(const uint8_t secret[32], uint8_t *ascr, AgreeOpen L, hipStream_t s);

// zero the key region of an agreement scratch: the last thing a call enqueues
hipError_t agree_wipe_enqueue(uint8_t *ascr, uint64_t count, hipStream_t s);

}  // namespace api
}  // namespace chip
