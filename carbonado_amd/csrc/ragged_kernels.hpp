// ragged_kernels.hpp — launch interface of ragged_kernels.hip (KR) for
// api_ragged.cpp.  The table it points to is laid out by ragged_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "ragged_plan.hpp"

namespace chip {

struct RaggedLaunch {
    const ragged::Obj *objs;  // device: [count]
    const uint32_t *groups;   // device: [count + 1] prefix of groups per object
    const uint32_t *blocks;   // device: [count + 1] prefix of parity / copy blocks per object
    uint8_t *gcv;             // device: [total_groups][32]
    uint64_t count, total_groups;
    uint64_t parity_blocks;   // encode with the Zfec bit
    uint64_t copy_blocks;     // decode at Zfec only
    bool bao, decode;
    uint8_t *hashes;          // Bao bit: [count][32] out (encode) or expected (decode)
    uint32_t *status;         // decode: [count], zero at launch
};

// Enqueue the kernels of one ragged call: parity or copy, groups, tops.
hipError_t ragged_launch(const RaggedLaunch &L, hipStream_t stream);

}  // namespace chip
