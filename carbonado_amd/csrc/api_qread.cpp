// api_qread.cpp — the device-planned ranged reads of
// include/carbonado_hip_qread.h.  chipq_stream_table_dev is the one upload of
// a set of resident streams (qread_plan.hpp: the per-stream checks of
// read::plan_read and the table).  The read calls do O(1) host work
// (qread::plan_call), fill the launch tables of KQ, KA, KD and KV with
// pointers into their own scratch and with bounds, and enqueue KQ's plan
// (qread_kernels.hip) and the launches of chipd_read_ranges_dev /
// chipv_read_ranges_dev behind it (api_read.hpp).  Kernels only: no upload, no
// memset, no synchronisation, no allocation after the thread's first call.
// read_planned is declared in api_qread.hpp: api_kread.cpp runs it over
// requests its own kernel rewrote.
#include "api_qread.hpp"

using namespace chip;
using namespace chip::api;

namespace chip {
namespace api {

int read_planned(const QreadCall &a, bool vouched) {
    if (a.nreq == 0) return CHIP_OK;
    qread::Geometry g;
    qread::ScratchLayout lay;
    int st = qread::plan_call(reinterpret_cast<uintptr_t>(a.d_table), a.info, a.d_req_stream && a.d_start && a.d_len,
                              a.nreq, a.max_len, reinterpret_cast<uintptr_t>(a.d_content), a.content_stride,
                              a.d_content_len && a.d_status && a.d_used && (!vouched || a.d_vouch), vouched, a.flags,
                              reinterpret_cast<uintptr_t>(a.d_scratch), a.scratch_len, &g, &lay);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    uint8_t *scr = static_cast<uint8_t *>(a.d_scratch);
    const uint8_t *table = static_cast<const uint8_t *>(a.d_table);

    QreadLaunch Q{};
    Q.recs = reinterpret_cast<const qread::StreamRec *>(table);
    Q.shape = qread::Shape{a.info->nstreams, a.info->max_chunks, a.info->min_shard, a.max_len, g.S};
    Q.req_stream = a.d_req_stream; Q.start = a.d_start; Q.len = a.d_len;
    Q.nreq = a.nreq;
    Q.content = reinterpret_cast<uint64_t>(a.d_content); Q.stride = a.content_stride;
    Q.tables.reqs = reinterpret_cast<read::Req *>(scr + lay.reqs);
    Q.tables.segs = reinterpret_cast<read::Seg *>(scr + lay.segs);
    Q.tables.slices = reinterpret_cast<audit::Req *>(scr + lay.slices);
    Q.tables.parents = reinterpret_cast<uint64_t *>(scr + lay.parents);
    Q.tables.chunks = reinterpret_cast<uint64_t *>(scr + lay.chunks);
    Q.tables.fpar = reinterpret_cast<uint64_t *>(scr + lay.fpar);
    Q.tables.blocks = reinterpret_cast<uint64_t *>(scr + lay.blocks);
    Q.tables.content_len = a.d_content_len;
    Q.pitch = lay.prefix_pitch / 8;
    Q.sums = reinterpret_cast<uint64_t *>(scr + lay.sums);
    Q.scan_blocks = g.scan_blocks;
    Q.rstat = reinterpret_cast<uint32_t *>(scr + lay.rstat);
    Q.pathw = vouched ? reinterpret_cast<uint32_t *>(scr + lay.path) : nullptr;
    Q.contra = vouched ? reinterpret_cast<uint32_t *>(scr + lay.contra) : nullptr;
    CHIP_HIP(qread_plan_launch(Q, s));

    // the launch tables of the older calls: every segment slot a segment, every total a bound
    AuditLaunch A{};
    A.reqs = Q.tables.slices; A.parents = Q.tables.parents; A.chunks = Q.tables.chunks;
    A.nreq = g.nslot; A.total_parents = g.parents; A.total_chunks = g.chunks;
    A.bounded = true;
    VreadLaunch V{};
    ReadLaunch &L = V.rd;
    L.slices = Q.tables.slices; L.parents = Q.tables.parents; L.chunks = Q.tables.chunks; L.fpar = Q.tables.fpar;
    L.masks = reinterpret_cast<const read::MaskEntry *>(table + qread::table_masks_off(a.info->nstreams));
    L.reqs = Q.tables.reqs; L.segs = Q.tables.segs; L.blocks = Q.tables.blocks;
    L.rstat = Q.rstat;
    L.served = reinterpret_cast<read::Served *>(scr + lay.served);
    L.nreq = a.nreq; L.nseg = g.nslot; L.total_blocks = g.blocks;
    L.prim_parents = g.parents; L.prim_chunks = g.chunks; L.fb_parents = g.fb_parents;
    L.status = a.d_status; L.used = a.d_used;
    L.bounded = true;
    if (!vouched) return read_enqueue_launches(L, A, s);
    V.pathw = Q.pathw;
    V.contra = Q.contra;
    V.vouch = a.d_vouch;
    V.strict = a.flags & CHIPV_STRICT;
    return vread_enqueue_launches(V, A, s);
}

}  // namespace api
}  // namespace chip

extern "C" {

int chipq_abi_version(void) { return CHIPQ_ABI_VERSION; }

uint64_t chipq_stream_table_len(uint64_t nstreams) { return qread::table_len(nstreams); }

int chipq_stream_table_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                           const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                           void *d_table, uint64_t table_len, chipq_table_info *info, void *stream) {
    std::vector<uint8_t> table;
    chipq_table_info out;
    int st = qread::plan_table(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len,
                               reinterpret_cast<uintptr_t>(d_hash), padding, chunk_len, nstreams,
                               reinterpret_cast<uintptr_t>(d_table), table_len, info ? &out : nullptr, &table);
    if (info) std::memset(info, 0, sizeof *info);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    CHIP_HIP(h2d(c->stage, d_table, table.data(), table.size(), static_cast<hipStream_t>(stream)));
    *info = out;
    return CHIP_OK;
}

uint64_t chipq_read_scratch_len(const chipq_table_info *info, uint64_t nreq, uint64_t max_len, uint32_t vouched) {
    return qread::scratch_len(info, nreq, max_len, vouched != 0);
}

int chipq_read_ranges_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                          const uint64_t *d_start, const uint64_t *d_len, uint64_t nreq, uint64_t max_len,
                          uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len, uint32_t *d_status,
                          uint32_t *d_used, void *d_scratch, uint64_t scratch_len, void *stream) {
    return read_planned(QreadCall{d_table, info, d_req_stream, d_start, d_len, nreq, max_len, d_content, content_stride,
                             d_content_len, d_status, d_used, nullptr, 0, d_scratch, scratch_len, stream},
                        false);
}

int chipq_read_ranges_vouched_dev(const void *d_table, const chipq_table_info *info, const uint32_t *d_req_stream,
                                  const uint64_t *d_start, const uint64_t *d_len, uint64_t nreq, uint64_t max_len,
                                  uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len,
                                  uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch, uint32_t flags,
                                  void *d_scratch, uint64_t scratch_len, void *stream) {
    return read_planned(QreadCall{d_table, info, d_req_stream, d_start, d_len, nreq, max_len, d_content, content_stride,
                             d_content_len, d_status, d_used, d_vouch, flags, d_scratch, scratch_len, stream},
                        true);
}

}  // extern "C"
