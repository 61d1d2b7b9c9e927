// vread_kernels.hpp — launch interface of vread_kernels.hip (KV) for
// api_vread.cpp.  The tables it points to are laid out by read_plan.hpp and
// vread_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "read_kernels.hpp"
#include "vread_plan.hpp"

namespace chip {

struct VreadLaunch {
    ReadLaunch rd;     // the ranged read's tables; rd.rstat[g] is segment g's chunk word
    uint32_t *pathw;   // device: [nseg] path word per segment, zero at launch
    uint32_t *contra;  // device: [nseg] contradiction word per segment, zero at launch
    uint32_t *vouch;   // the caller's: [nreq]
    uint32_t strict;   // flags & CHIPV_STRICT
};

// Enqueue the class per segment and the gated hashing of the rebuilt window
// chunks (two launches, behind read_fallback_launch with the path words).
hipError_t vread_vouch_launch(const VreadLaunch &L, hipStream_t stream);

// Enqueue the verdict per request: status, used and vouch (one launch).  The
// read itself follows with read_copy_launch.
hipError_t vread_finish_launch(const VreadLaunch &L, hipStream_t stream);

}  // namespace chip
