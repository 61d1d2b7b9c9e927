// api_cread.hpp — the enqueue half of chipc_ctr_ranges_dev (api_cread.cpp) for
// the calls that run the keystream inside their own (api_fread.cpp).
#pragma once

#include "api_common.hpp"
#include "cread_plan.hpp"

namespace chip {
namespace api {

// Everything chipc_ctr_ranges_dev does behind its host checks: the table of a
// plan that cread::plan_ctr accepted, uploaded into d_scratch through the
// pinned copy, the two launches and the memset that zeroes the key region, on
// `stream`.  d_status, d_used, d_vouch: the read's words, written for killed
// items only (NULL where the plan has none).  Does not synchronise.
int ctr_enqueue(cread::Plan &p, uint8_t *d_buf, const uint32_t *d_gate, uint32_t *d_status, uint32_t *d_used,
                uint32_t *d_vouch, void *d_scratch, void *stream);

}  // namespace api
}  // namespace chip
