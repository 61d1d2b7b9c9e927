// api_kread.hpp — the whole of chipk_read_ranges_dev (api_kread.cpp) for the
// calls that run a device-planned level-13 read inside their own
// (api_gread.cpp).
#pragma once

#include "api_qread.hpp"
#include "kread_kernels.hpp"

namespace chip {
namespace api {

// The arguments of chipk_read_ranges_dev, as its header lists them: a planned
// read call's, with the key table.
struct KreadCall {
    QreadCall q;
    const void *d_keytab;
    uint64_t keytab_len;
};

// Everything chipk_read_ranges_dev does: the host checks (kread::plan_call),
// KK's rewrite, read_planned over the rewritten requests and KK's keystream
// launch, 14 launches on a.q.stream.  Kernels only; does not synchronise.
int read_plain_planned(const KreadCall &a);

}  // namespace api
}  // namespace chip
