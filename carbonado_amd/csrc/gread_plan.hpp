// gread_plan.hpp — host side of the device-planned plaintext reads of level-14
// and level-15 objects (include/carbonado_hip_gread.h): the frame table's
// layout, checks and one upload, and the O(1) host work of a read call
// (argument checks in the header's order, the inner capacity, the block grid,
// the scratch layout).  The requests are decided on the device
// (gread_device.hpp, gread_kernels.hip); the host never sees them.
// Pure host code without a HIP type in it (tests/gread_plan_check.cpp drives it
// under a sanitizer).
#pragma once

#include "../../include/carbonado_hip_gread.h"
#include "fread_plan.hpp"
#include "gread_device.hpp"
#include "kread_plan.hpp"

namespace chip {
namespace gread {

using read::up;

// ---- the frame table ---------------------------------------------------------------
// [nstreams FrameRec (32 B each) | the entries, 8 B each], the entries on a 16-B
// boundary (32 nstreams is one).  The entries are those of the streams whose
// index_status is 0, nframes + 1 each, compacted in stream order: stream s has
// entries [ent0, ent0 + nframes] of them.  A stream whose index_status is not 0
// has ent0 = nframes = 0 and no entry.
struct TableLayout {
    uint64_t recs = 0, entries = 0, total = 0;
    TableLayout() {}
    TableLayout(uint64_t nstreams, uint64_t nentries) {
        entries = nstreams * sizeof(FrameRec);
        total = entries + fread::up16(nentries * 8);
    }
};

inline uint64_t table_len(uint64_t nstreams, uint64_t nentries) {
    if (nstreams >= fread::MAX_STREAMS || nentries >= fread::MAX_ENTRIES) return 0;
    return TableLayout(nstreams, nentries).total;
}

// The host checks of chipg_frame_table_dev in the header's order (everything but
// the device), chipg_frame_info and the table as uploaded.  The per-stream
// checks are fread::check_reads', in its order.
inline int plan_table(uint8_t format, const uint32_t *chunk_len, const uint32_t *padding, const uint32_t *index_status,
                      const uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *nframes,
                      const uint64_t *plain_len, uint64_t nstreams, uintptr_t d_ftable, uint64_t ftable_len,
                      chipg_frame_info *finfo, std::vector<uint8_t> *table) {
    if (!finfo) return CHIP_ERR_INVALID_ARG;
    std::memset(finfo, 0, sizeof *finfo);
    table->clear();
    if (!fread::format_ok(format)) return CHIP_ERR_INVALID_ARG;
    if (nstreams == 0) {
        finfo->format = format;
        return CHIP_OK;
    }
    if (!chunk_len || !padding || !frame_off || !idx_off || !nframes || !plain_len || !d_ftable)
        return CHIP_ERR_INVALID_ARG;
    if (nstreams >= fread::MAX_STREAMS) return CHIP_ERR_INVALID_ARG;
    const int st = fread::check_reads(format, 0, chunk_len, padding, frame_off, idx_off, nframes, plain_len,
                                      index_status, nstreams, nullptr, nullptr, nullptr, 0);
    if (st != CHIP_OK) return st;
    uint64_t ne = 0, max_frame = 0;
    for (uint64_t s = 0; s < nstreams; ++s) {
        if (index_status && index_status[s]) continue;
        ne += nframes[s] + 1;  // below 2^31 each, 2^31 streams at most
        const uint64_t *off = frame_off + idx_off[s];
        for (uint64_t f = 0; f < nframes[s]; ++f) max_frame = std::max(max_frame, off[f + 1] - off[f]);
    }
    if (ne >= fread::MAX_ENTRIES || d_ftable % 16 || ftable_len < table_len(nstreams, ne)) return CHIP_ERR_INVALID_ARG;
    const TableLayout lay(nstreams, ne);
    table->assign(lay.total, 0);
    uint64_t e = 0;
    for (uint64_t s = 0; s < nstreams; ++s) {
        FrameRec r{};
        r.plain_len = plain_len[s];
        r.index_status = index_status ? index_status[s] : 0;
        if (!r.index_status) {
            r.ent0 = e;
            r.nframes = nframes[s];
            std::memcpy(table->data() + lay.entries + 8 * e, frame_off + idx_off[s], 8 * (nframes[s] + 1));
            e += nframes[s] + 1;
        }
        std::memcpy(table->data() + lay.recs + s * sizeof r, &r, sizeof r);
    }
    finfo->nstreams = nstreams;
    finfo->nentries = ne;
    finfo->max_frame = max_frame;
    finfo->format = format;
    return CHIP_OK;
}

// ---- a read call ---------------------------------------------------------------------
constexpr uint64_t MAX_WORK = uint64_t(1) << 31;    // workgroups of the block decode
constexpr uint64_t MAX_STAGE = uint64_t(1) << 62;   // bytes of all staging slots

// The inner planned read runs over (nreq, max_len') with max_len' = fcap
// max_frame: a request of max_len plaintext bytes or fewer touches fcap frames
// or fewer, each of max_frame frame-stream bytes or fewer.  A table without a
// frame (max_frame 0) still serves its empty and killed requests: the inner
// capacity is 1 byte then, since the inner call takes no capacity of 0.
struct Geometry {
    uint64_t fcap = 0, inner_len = 0, stage_stride = 0, work = 0;
    bool keyed = false, ok = false;
    qread::Geometry q;  // of the inner read
    uint64_t inner_scratch = 0;
    Geometry() {}
    Geometry(const chipq_table_info &info, const chipg_frame_info &finfo, uint64_t nreq, uint64_t max_len) {
        keyed = finfo.format == 15;
        fcap = fcap_of(max_len);
        const unsigned __int128 il = (unsigned __int128)fcap * finfo.max_frame;
        if (il > read::MAX_RANGE) return;
        inner_len = il ? (uint64_t)il : 1;
        stage_stride = fread::up16(inner_len);
        const unsigned __int128 w = (unsigned __int128)nreq * fcap, st = (unsigned __int128)nreq * stage_stride;
        if (w >= MAX_WORK || st > MAX_STAGE) return;
        work = (uint64_t)w;
        inner_scratch = keyed ? kread::scratch_len(&info, nreq, inner_len) : qread::scratch_len(&info, nreq, inner_len, true);
        if (!inner_scratch) return;
        q = qread::Geometry(info, nreq, inner_len);
        ok = q.ok;
    }
};

// [the inner call's scratch | the rewritten requests: stream, start, len | the
// inner call's content lengths | a verdict word per (request, k) | the staging
// slots, nreq of stage_stride bytes], every region on a 256-B boundary.  Nothing
// here depends on a key.
struct ScratchLayout {
    uint64_t inner = 0, inner_len = 0, q_stream = 0, q_start = 0, q_len = 0, q_clen = 0, bad = 0, stage = 0, total = 0;
    ScratchLayout() {}
    ScratchLayout(const Geometry &g, uint64_t nreq) {
        inner_len = g.inner_scratch;
        q_stream = up(inner_len, 256);
        q_start = q_stream + up(nreq * 4, 256);
        q_len = q_start + up(nreq * 8, 256);
        q_clen = q_len + up(nreq * 8, 256);
        bad = q_clen + up(nreq * 8, 256);
        stage = bad + up(g.work * 4, 256);
        total = stage + nreq * g.stage_stride;
    }
};

inline bool format_ok(const chipg_frame_info *finfo) { return finfo && (finfo->format == 14 || finfo->format == 15); }

inline uint64_t scratch_len(const chipq_table_info *info, const chipg_frame_info *finfo, uint64_t nreq, uint64_t max_len) {
    if (!info || !format_ok(finfo) || nreq >= (1ull << 31) || !qread::range_ok(max_len)) return 0;
    if (finfo->nstreams != info->nstreams) return 0;
    if (finfo->format == 15 ? !kread::scratch_len(info, nreq, max_len) : !qread::scratch_len(info, nreq, max_len, true))
        return 0;
    const Geometry g(*info, *finfo, nreq, max_len);
    return g.ok ? ScratchLayout(g, nreq).total : 0;
}

// the inner planned call's host checks over capacity (nreq, max_len, content_stride), any scratch length
inline int inner_checks(bool keyed, uintptr_t d_table, const chipq_table_info *info, uintptr_t d_keytab,
                        uint64_t keytab_len, bool have_requests, uint64_t nreq, uint64_t max_len, uintptr_t d_content,
                        uint64_t content_stride, bool have_results, uint32_t flags, uintptr_t d_scratch) {
    qread::Geometry qg;
    qread::ScratchLayout ql;
    kread::Geometry kg;
    kread::ScratchLayout kl;
    if (keyed)
        return kread::plan_call(d_table, info, d_keytab, keytab_len, have_requests, nreq, max_len, d_content,
                                content_stride, have_results, flags, d_scratch, ~0ull, &kg, &kl);
    return qread::plan_call(d_table, info, have_requests, nreq, max_len, d_content, content_stride, have_results, true,
                            flags, d_scratch, ~0ull, &qg, &ql);
}

// The host checks of chipg_read_ranges_dev, in the header's order; everything but the device.
inline int plan_call(uintptr_t d_table, const chipq_table_info *info, uintptr_t d_ftable, const chipg_frame_info *finfo,
                     uintptr_t d_keytab, uint64_t keytab_len, bool have_requests, uint64_t nreq, uint64_t max_len,
                     uintptr_t d_content, uint64_t content_stride, bool have_results, uint32_t flags,
                     uintptr_t d_scratch, uint64_t scratch_len_given, Geometry *g, ScratchLayout *lay) {
    if (nreq == 0) return CHIP_OK;
    if (!d_table || !info || !d_ftable || !finfo || !have_requests || !d_content || !have_results || !d_scratch)
        return CHIP_ERR_INVALID_ARG;
    if (!format_ok(finfo)) return CHIP_ERR_INVALID_ARG;
    const bool keyed = finfo->format == 15;
    if (keyed && !d_keytab) return CHIP_ERR_INVALID_ARG;
    int st = inner_checks(keyed, d_table, info, d_keytab, keytab_len, true, nreq, max_len, d_content, content_stride,
                          true, flags, d_scratch);
    if (st != CHIP_OK) return st;
    *g = Geometry(*info, *finfo, nreq, max_len);
    if (!g->ok) return CHIP_ERR_INVALID_ARG;
    *lay = ScratchLayout(*g, nreq);
    st = inner_checks(keyed, d_table, info, d_keytab, keytab_len, true, nreq, g->inner_len, d_scratch + lay->stage,
                      g->stage_stride, true, flags, d_scratch);
    if (st != CHIP_OK) return st;
    if (d_ftable % 16) return CHIP_ERR_INVALID_ARG;
    if (finfo->nstreams != info->nstreams) return CHIP_ERR_INVALID_ARG;
    // (2^31 or more block workgroups: Geometry)
    if (scratch_len_given < lay->total) return CHIP_ERR_INVALID_ARG;
    return CHIP_OK;
}

// The Shape the kernels decide by.
inline Shape shape_of(const chipq_table_info &info, const chipg_frame_info &finfo, uint64_t max_len, const Geometry &g) {
    Shape sh;
    sh.nstreams = finfo.nstreams;
    sh.nentries = finfo.nentries;
    sh.max_frame = finfo.max_frame;
    sh.max_len = max_len;
    sh.fcap = uint32_t(g.fcap);
    sh.keyed = g.keyed ? 1 : 0;
    sh.inner = qread::Shape{info.nstreams, info.max_chunks, info.min_shard, g.inner_len, g.q.S};
    return sh;
}

}  // namespace gread
}  // namespace chip
