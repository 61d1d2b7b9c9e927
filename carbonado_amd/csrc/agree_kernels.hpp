// agree_kernels.hpp — launch interface of agree_kernels.hip (KY) for
// api_agree.cpp.  The scratch regions it points to are laid out by
// agree_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "agree_device.hpp"

namespace chip {

// E = k G, key = HKDF(E65 || (k P)65) of every object: one wave each.
struct AgreeSeal {
    const uint32_t *gtab;  // device: the comb table of G
    const uint32_t *ptab;  // device: the comb table of the receiver's key P
    const uint32_t *sk;    // device, key region: [count] scalars of eight little-endian words
    uint32_t count;
    uint8_t *pub;          // object o's 65 bytes at pub + o pub_pitch
    uint64_t pub_pitch;
    uint8_t *keys;         // object o's 32 bytes at keys + o key_pitch
    uint64_t key_pitch;
};
hipError_t agree_seal_launch(const AgreeSeal &L, hipStream_t stream);

// key = HKDF(R65 || (sk R)65) of every object: one lane each.
struct AgreeOpen {
    const uint32_t *sk;    // device, key region: the receiver's scalar, eight little-endian words
    uint32_t *vtab;        // device: agree::var_words(count) words for the tables of multiples
    uint32_t count;
    const uint8_t *eph;    // object o's 65 bytes at eph + o eph_pitch
    uint64_t eph_pitch;
    uint8_t *keys;         // object o's 32 bytes at keys + o key_pitch (zeros for a key that does not parse)
    uint64_t key_pitch;
    uint32_t *status;      // [count]: 0 or 17; or NULL
    uint8_t *refused;      // or NULL: the uint32 at refused + o refused_stride is set to 1 for a key that does not parse
    uint64_t refused_stride;
    uint32_t copy_iv;      // the 16 bytes behind an ephemeral key are copied behind its AES key
    // optional, public: words that fail object o before its key is looked at.  gate[o] != 0: that status (the
    // status of the read that fetched its header); shorter[o] != 0: 17 whatever gate says.  A failed object's
    // key (and, with copy_iv, nonce) is zeros.
    const uint32_t *gate;
    const uint32_t *shorter;
};
hipError_t agree_open_launch(const AgreeOpen &L, hipStream_t stream);


// One request per stream of a qread stream table for the key table call:
// envelope bytes [0, 81) of stream s, or nothing (and shorter[s] = 1) of an
// object too short to be an envelope (4 C - padding < 97).
struct AgreeRequests {
    const void *recs;  // device: [nstreams] qread::StreamRec
    uint32_t nstreams;
    uint32_t *req_stream;
    uint64_t *start, *len;
    uint32_t *shorter;
};
hipError_t agree_requests_launch(const AgreeRequests &L, hipStream_t stream);

}  // namespace chip
