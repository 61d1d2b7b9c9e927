// cread_kernels.hpp — launch interface of cread_kernels.hip (KC) for
// api_cread.cpp.  The tables it points to are laid out by cread_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "cread_device.hpp"

namespace chip {

struct CtrLaunch {
    const cread::Item *items;  // device: [nitems]
    const uint8_t *rawkeys;    // device: [keys_used] key (32) || IV (16)
    cread::CtrKey *km;         // device: [keys_used]
    uint32_t nitems, keys_used, work;
    uint8_t *buf;              // the ranges, XORed in place
    const uint32_t *gate;      // device: [nitems] or NULL: item i is skipped when gate[i] != 0
    uint32_t *status, *used, *vouch;  // the read's result words: written for killed items only
};

// Round keys and J0 of every key of the table: one wave each.
hipError_t ctr_setup_launch(const CtrLaunch &L, hipStream_t stream);
// One wave per work item (item, span of 127 units): keystream XORed over the
// span, gated; zeros and the status words for a killed item.
hipError_t ctr_range_launch(const CtrLaunch &L, hipStream_t stream);

}  // namespace chip
