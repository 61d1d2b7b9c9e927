// snap_kernels.hpp — launch interface of snap_kernels.hip (KZ) for
// api_snap.cpp.  The tables it points to are laid out by snap_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "snap_device.hpp"

namespace chip {

struct SnapLaunch {
    const snap::CObj *objs;  // device: [count]
    const snap::CBlk *blks;  // device: [blocks]
    snap::CMeta *meta;       // device: [blocks]
    uint8_t *slots;          // device: [blocks] of snap::SLOT_PITCH bytes
    uint32_t count, blocks;
    const uint8_t *in;
    uint8_t *out;
    uint64_t *out_len;  // device: [count]
};

// One wave per 64 KiB block: the block compressed into its slot, its length
// and masked CRC into meta.
hipError_t snap_block_launch(const SnapLaunch &L, hipStream_t stream);
// One lane per object: FrameEncoder's raw rule, the chunk offsets, out_len.
hipError_t snap_frame_launch(const SnapLaunch &L, hipStream_t stream);
// One workgroup per block: stream identifier, chunk header and body at their byte offsets.
hipError_t snap_gather_launch(const SnapLaunch &L, hipStream_t stream);

struct UnsnapLaunch {
    const snap::UObj *objs;    // device: [count]
    const uint32_t *slot_obj;  // device: [slots]
    snap::UDesc *desc;         // device: [slots]
    uint32_t *bad;             // device: [slots] a block that does not decode or whose CRC disagrees
    snap::UState *state;       // device: [count]
    uint32_t count, slots;
    const uint8_t *in;
    uint8_t *out;
    uint64_t *out_len;    // device: [count]
    uint32_t *status;     // device: [count]
    uint32_t keep_status; // a stream whose status word is already non-zero keeps it and is not touched
};

// One lane per stream: the framing checked in the host's order, block descriptors, needed length, status.
hipError_t unsnap_walk_launch(const UnsnapLaunch &L, hipStream_t stream);
// One wave per slot, gated on the walk: the block decoded in LDS and stored (a raw chunk copied).
hipError_t unsnap_block_launch(const UnsnapLaunch &L, hipStream_t stream);
// One wave per slot: CRC-32C of the stored block against the chunk's word.
hipError_t unsnap_crc_launch(const UnsnapLaunch &L, hipStream_t stream);
// One workgroup per stream: the blocks' verdicts combined; a failed stream zeroed.
hipError_t unsnap_finish_launch(const UnsnapLaunch &L, hipStream_t stream);

}  // namespace chip
