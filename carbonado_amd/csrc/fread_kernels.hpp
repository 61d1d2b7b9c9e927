// fread_kernels.hpp — launch interface of fread_kernels.hip (KF) for
// api_fread.cpp.  The tables it points to are laid out by fread_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "fread_device.hpp"

namespace chip {

struct WalkLaunch {
    const fread::WStream *streams;  // device: [count]
    const cread::CtrKey *km;        // device: [count], read where a stream's shift != 0
    const uint8_t *in;              // d_streams
    fread::WalkOut *out;            // device: [count]
    uint64_t *off;                  // device: the call's entries
    uint32_t count;
};

// One lane per stream: the chunk headers followed serially from the primary
// copy, the offsets and what the walk found.
hipError_t fread_walk_launch(const WalkLaunch &L, hipStream_t stream);

struct ChainLaunch {
    const fread::VStream *streams;  // device: [count]
    const uint64_t *off;            // device: the uploaded entries
    const uint8_t *rows;            // device: 16 B per entry, the staged header bytes
    const uint32_t *rstat, *rvouch; // device: the header reads' words
    uint32_t *status;               // device: [count]
    uint64_t *plain;                // device: [count]
    uint32_t *vouch;                // device: [count]
    uint32_t count;
};

// One wave per stream: every link of its index checked against the staged headers.
hipError_t fread_chain_launch(const ChainLaunch &L, hipStream_t stream);

struct FrameLaunch {
    const fread::Req *reqs;  // device: [nreq]
    const fread::Seg *segs;  // device: [nseg]
    uint32_t *bad;           // device: [nseg]
    const uint8_t *rows;     // device: the staging rows
    uint8_t *content;
    uint32_t *status, *used, *vouch;  // device: [nreq], the vouched read's
    uint32_t nreq, nseg;
};

// One wave per (request, frame), gated on the read's status: header against
// the index, block decode in LDS, CRC, the wanted bytes stored.
hipError_t fread_block_launch(const FrameLaunch &L, hipStream_t stream);
// One workgroup per request: the frames' verdicts combined; a failed or killed request zeroed.
hipError_t fread_finish_launch(const FrameLaunch &L, hipStream_t stream);

}  // namespace chip
