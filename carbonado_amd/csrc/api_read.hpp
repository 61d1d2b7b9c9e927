// api_read.hpp — the enqueue halves of chipd_read_ranges_dev (api_read.cpp) and
// chipv_read_ranges_dev (api_vread.cpp) behind the table upload, for the calls
// whose tables are written on the device (api_qread.cpp).
#pragma once

#include "api_common.hpp"
#include "audit_kernels.hpp"
#include "vread_kernels.hpp"

namespace chip {
namespace api {

// Everything chipd_read_ranges_dev enqueues behind its upload and its memset
// of the status words, from a launch table: KA's checks of the segments' own
// slices (A: the slice requests as KA's table; its status, proofs and units are
// set here), the gated fallback checks, the verdicts and the read (6 launches).
// The status words (L.rstat) are zero when the first launch runs.  Does not
// synchronise.
int read_enqueue_launches(const ReadLaunch &L, AuditLaunch A, hipStream_t s);

// The same for chipv_read_ranges_dev: its 8 launches; the status, path and
// contradiction words are zero when the first one runs.
int vread_enqueue_launches(const VreadLaunch &V, AuditLaunch A, hipStream_t s);

}  // namespace api
}  // namespace chip
