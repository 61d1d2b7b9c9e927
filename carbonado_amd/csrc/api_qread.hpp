// api_qread.hpp — the enqueue half of chipq_read_ranges_dev and
// chipq_read_ranges_vouched_dev (api_qread.cpp) for the calls that run a
// device-planned read inside their own (api_kread.cpp).
#pragma once

#include "api_read.hpp"
#include "qread_kernels.hpp"

namespace chip {
namespace api {

// The arguments of a device-planned read call, as its header lists them.
struct QreadCall {
    const void *d_table;
    const chipq_table_info *info;
    const uint32_t *d_req_stream;
    const uint64_t *d_start, *d_len;
    uint64_t nreq, max_len;
    uint8_t *d_content;
    uint64_t content_stride;
    uint64_t *d_content_len;
    uint32_t *d_status, *d_used, *d_vouch;
    uint32_t flags;
    void *d_scratch;
    uint64_t scratch_len;
    void *stream;
};

// Everything a chipq_ read call does: the host checks (qread::plan_call), KQ's
// 4 planning launches and the 6 launches of chipd_read_ranges_dev or (vouched)
// the 8 of chipv_read_ranges_dev, on a.stream.  Kernels only; does not
// synchronise.
int read_planned(const QreadCall &a, bool vouched);

}  // namespace api
}  // namespace chip
