// repair_kernels.hpp — launch interface of repair_kernels.hip (KP) for
// api_repair.cpp.  The tables it points to are laid out by repair_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "repair_plan.hpp"

namespace chip {

// masks[o] = bit i set when status word first[o] + i is 0, for the
// first[o + 1] - first[o] (8 or 0) requests of object o (one launch).
hipError_t repair_fold_launch(const uint32_t *rstat, const uint32_t *first, uint32_t count, uint32_t *masks,
                              hipStream_t stream);

// zfec-decode every record's 4 selected shares, read in their chunk slots of
// the damaged stream, to its 4 primaries (one launch).
hipError_t repair_decode_launch(const repair::Rec *recs, const uint32_t *blocks, uint32_t nrep, uint64_t total_blocks,
                                hipStream_t stream);

// ok[j] = the re-encoded hash of repair j equals the expected one, then every
// row whose ok is set copied to its output range (two launches).
hipError_t repair_commit_launch(const repair::Commit *commits, const uint64_t *units, uint32_t nrep,
                                uint64_t total_units, uint32_t *ok, hipStream_t stream);

}  // namespace chip
