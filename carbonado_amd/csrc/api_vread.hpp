// api_vread.hpp — the enqueue half of chipv_read_ranges_dev (api_vread.cpp) for
// the calls that run a vouched read inside their own (api_cread.cpp).
#pragma once

#include "api_common.hpp"
#include "vread_plan.hpp"

namespace chip {
namespace api {

// Everything chipv_read_ranges_dev does behind its host checks: the table of a
// plan that vread::plan_vread accepted, uploaded into d_scratch, the memset and
// the launches, on `stream`.  Does not synchronise.
int vread_enqueue(vread::Plan &vp, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch, uint32_t flags,
                  void *d_scratch, void *stream);

}  // namespace api
}  // namespace chip
