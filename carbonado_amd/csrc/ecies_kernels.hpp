// ecies_kernels.hpp — launch interface of ecies_kernels.hip (KE) for
// api_ecies.cpp.  The tables it points to are laid out by ecies_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "gcm_device.hpp"

namespace chip {

struct GcmLaunch {
    const gcm::Msg *msgs;    // device: [count]
    const uint8_t *rawkeys;  // device: [count] key (32) || IV (16)
    gcm::KeyMat *km;         // device: [count]
    gcm::B128 *vals;         // device: [items]
    uint32_t *ok;            // device: [count] verdict words (open)
    uint32_t count, items;
    const uint8_t *in;       // plaintext (seal) or ciphertext (open)
    uint8_t *out;            // ciphertext (seal) or plaintext (open)
    uint8_t *tag;            // written by a seal, only read by an open
    uint32_t *status;        // the caller's: [count] (open)
    uint32_t keep_status;    // open: a message whose status word is already non-zero keeps it and fails
};

// Round keys, powers of H, J0 and E_K(J0) of every message: one wave each.
hipError_t gcm_setup_launch(const GcmLaunch &L, hipStream_t stream);
// The 81 header bytes in front of every message's tag (L.tag + tag_off - 81):
// from the 96-B slots at hdrs into the envelopes (scatter) or back.  Messages
// marked refused are skipped.
hipError_t gcm_hdr_launch(const GcmLaunch &L, uint8_t *hdrs, bool scatter, hipStream_t stream);
// One wave per item: gcm::MODE_SEAL (CTR + GHASH), MODE_HASH (GHASH of the
// ciphertext) or MODE_CTR (the pass of an open, gated on the verdict words).
hipError_t gcm_span_launch(const GcmLaunch &L, uint32_t mode, hipStream_t stream);
// One wave per message: the tag from the items' values, written (seal) or
// compared with the one given, into the verdict and status words (open).
hipError_t gcm_finish_launch(const GcmLaunch &L, bool seal, hipStream_t stream);

}  // namespace chip
