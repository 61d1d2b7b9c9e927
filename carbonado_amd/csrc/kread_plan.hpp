// kread_plan.hpp — host side of the device-planned plaintext reads of level-13
// objects (include/carbonado_hip_kread.h): the key table's layout and checks,
// and the O(1) host work of a read call (argument checks in the header's order,
// the keystream grid, the scratch layout).  The requests are decided on the
// device (kread_device.hpp, kread_kernels.hip); the host never sees them.
// Pure host code without a HIP type in it (tests/kread_plan_check.cpp drives it
// under a sanitizer).
#pragma once

#include "../../include/carbonado_hip_kread.h"
#include "cread_plan.hpp"
#include "kread_device.hpp"
#include "qread_plan.hpp"

namespace chip {
namespace kread {

using read::up;

// ---- the key table -----------------------------------------------------------------
// [nstreams cread::CtrKey | nstreams key_status words | nstreams raw records],
// every region 16-B aligned.  The words and the raw records are one upload; the
// raw records are the staging part, zeros once chipk_key_table_dev's work is done.
struct TableLayout {
    uint64_t km = 0, status = 0, raw = 0, total = 0;
    TableLayout() {}
    explicit TableLayout(uint64_t nstreams) {
        status = nstreams * sizeof(cread::CtrKey);
        raw = status + cread::up16(nstreams * 4);
        total = raw + nstreams * cread::RAW_KEY;
    }
    uint64_t upload_len() const { return total - status; }
};

inline uint64_t table_len(uint64_t nstreams) {
    if (nstreams >= (1ull << 32)) return 0;  // a request names its stream in 32 bits
    return TableLayout(nstreams).total;
}

// The host checks of chipk_key_table_dev, in the header's order; everything but the device.
inline int check_table(bool have_keys, bool have_ivs, uintptr_t d_keytab, uint64_t nstreams, uint64_t keytab_len) {
    if (nstreams == 0) return CHIP_OK;
    if (!have_keys || !have_ivs || !d_keytab || d_keytab % 16 || nstreams >= (1ull << 32) ||
        keytab_len < table_len(nstreams))
        return CHIP_ERR_INVALID_ARG;
    return CHIP_OK;
}

// What chipk_key_table_dev uploads behind the records: the key_status words and
// key || IV of every stream, zeros for a stream whose word is not 0.  It holds
// keys: the caller wipes it.
inline std::vector<uint8_t> table_upload(const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status,
                                         uint64_t nstreams) {
    const TableLayout lay(nstreams);
    std::vector<uint8_t> t(lay.upload_len(), 0);
    uint8_t *raw = t.data() + (lay.raw - lay.status);
    for (uint64_t s = 0; s < nstreams; ++s) {
        const uint32_t ks = key_status ? key_status[s] : 0;
        std::memcpy(t.data() + 4 * s, &ks, 4);
        if (ks) continue;
        std::memcpy(raw + cread::RAW_KEY * s, keys + 32 * s, 32);
        std::memcpy(raw + cread::RAW_KEY * s + 32, ivs + 16 * s, 16);
    }
    return t;
}

// ---- a read call ---------------------------------------------------------------------
constexpr uint64_t MAX_WORK = uint64_t(1) << 31;  // waves of the keystream kernel

struct Geometry {
    qread::Geometry q;
    uint32_t cap = 0;   // spans per request: cread::spans_of(max_len)
    uint64_t work = 0;  // nreq cap: one wave each
    bool ok = false;
    Geometry() {}
    Geometry(const chipq_table_info &info, uint64_t nreq, uint64_t max_len) : q(info, nreq, max_len) {
        const unsigned __int128 w = (unsigned __int128)nreq * cread::spans_of(max_len);
        ok = q.ok && w < MAX_WORK;
        if (!ok) return;
        cap = span_cap(max_len);
        work = (uint64_t)w;
    }
};

// [qread's vouched scratch | the rewritten requests: stream, start, len], every
// region on a 256-B boundary.  Nothing here depends on a key.
struct ScratchLayout {
    qread::ScratchLayout q;
    uint64_t q_stream = 0, q_start = 0, q_len = 0, total = 0;
    ScratchLayout() {}
    ScratchLayout(const Geometry &g, uint64_t nreq) : q(g.q, nreq, true) {
        q_stream = up(q.total, 256);
        q_start = q_stream + up(nreq * 4, 256);
        q_len = q_start + up(nreq * 8, 256);
        total = q_len + up(nreq * 8, 256);
    }
};

inline uint64_t scratch_len(const chipq_table_info *info, uint64_t nreq, uint64_t max_len) {
    if (!info || nreq >= (1ull << 31) || !qread::range_ok(max_len)) return 0;
    const Geometry g(*info, nreq, max_len);
    return g.ok ? ScratchLayout(g, nreq).total : 0;
}

// The host checks of chipk_read_ranges_dev, in the header's order: qread's, with
// the key table where it reports a bad d_table and kread's scratch length in the
// place of its own.
inline int plan_call(uintptr_t d_table, const chipq_table_info *info, uintptr_t d_keytab, uint64_t keytab_len,
                     bool have_requests, uint64_t nreq, uint64_t max_len, uintptr_t d_content,
                     uint64_t content_stride, bool have_results, uint32_t flags, uintptr_t d_scratch,
                     uint64_t scratch_len_given, Geometry *g, ScratchLayout *lay) {
    if (nreq == 0) return CHIP_OK;
    if (!d_keytab) return CHIP_ERR_INVALID_ARG;
    qread::Geometry qg;
    qread::ScratchLayout ql;
    const int st = qread::plan_call(d_table, info, have_requests, nreq, max_len, d_content, content_stride,
                                    have_results, true, flags, d_scratch, ~0ull, &qg, &ql);
    if (st != CHIP_OK) return st;
    if (d_keytab % 16 || info->nstreams >= (1ull << 32) || keytab_len < table_len(info->nstreams))
        return CHIP_ERR_INVALID_ARG;
    *g = Geometry(*info, nreq, max_len);
    if (!g->ok) return CHIP_ERR_INVALID_ARG;
    *lay = ScratchLayout(*g, nreq);
    if (scratch_len_given < lay->total) return CHIP_ERR_INVALID_ARG;
    return CHIP_OK;
}

}  // namespace kread
}  // namespace chip
