// api_gread.cpp — the device-planned plaintext reads of level-14 and level-15
// objects of include/carbonado_hip_gread.h.  chipg_frame_table_dev is the one
// upload of the frame indexes of a set of resident streams (gread_plan.hpp: the
// per-stream checks of fread::check_reads and the table).  A read call does
// O(1) host work (gread::plan_call) and enqueues KG's rewrite, the inner planned
// read of the rewritten requests into staging slots of its own scratch
// (read_planned of api_qread.hpp at 14, read_plain_planned of api_kread.hpp at
// 15), KG's block decode and KG's finish.  Kernels only: no upload, no memset,
// no synchronisation, no allocation after the thread's first call.
#include "api_kread.hpp"
#include "gread_kernels.hpp"

using namespace chip;
using namespace chip::api;

extern "C" {

int chipg_abi_version(void) { return CHIPG_ABI_VERSION; }

uint64_t chipg_frame_table_len(uint64_t nstreams, uint64_t nentries) { return gread::table_len(nstreams, nentries); }

int chipg_frame_table_dev(uint8_t format, const uint32_t *chunk_len, const uint32_t *padding,
                          const uint32_t *index_status, const uint64_t *frame_off, const uint64_t *idx_off,
                          const uint64_t *nframes, const uint64_t *plain_len, uint64_t nstreams, void *d_ftable,
                          uint64_t ftable_len, chipg_frame_info *finfo, void *stream) {
    std::vector<uint8_t> table;
    chipg_frame_info out;
    int st = gread::plan_table(format, chunk_len, padding, index_status, frame_off, idx_off, nframes, plain_len,
                               nstreams, reinterpret_cast<uintptr_t>(d_ftable), ftable_len, finfo ? &out : nullptr,
                               &table);
    if (finfo) std::memset(finfo, 0, sizeof *finfo);
    if (st != CHIP_OK) return st;
    if (!table.empty()) {
        st = use_device();
        if (st != CHIP_OK) return st;
        Ctx *c;
        st = ctx_get(&c);
        if (st != CHIP_OK) return st;
        CHIP_HIP(h2d(c->stage, d_ftable, table.data(), table.size(), static_cast<hipStream_t>(stream)));
    }
    *finfo = out;
    return CHIP_OK;
}

uint64_t chipg_read_scratch_len(const chipq_table_info *info, const chipg_frame_info *finfo, uint64_t nreq,
                                uint64_t max_len) {
    return gread::scratch_len(info, finfo, nreq, max_len);
}

int chipg_read_ranges_dev(const void *d_table, const chipq_table_info *info, const void *d_ftable,
                          const chipg_frame_info *finfo, const void *d_keytab, uint64_t keytab_len,
                          const uint32_t *d_req_stream, const uint64_t *d_start, const uint64_t *d_len, uint64_t nreq,
                          uint64_t max_len, uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len,
                          uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch, uint32_t flags, void *d_scratch,
                          uint64_t scratch_len, void *stream) {
    if (nreq == 0) return CHIP_OK;
    gread::Geometry g;
    gread::ScratchLayout lay;
    int st = gread::plan_call(reinterpret_cast<uintptr_t>(d_table), info, reinterpret_cast<uintptr_t>(d_ftable), finfo,
                              reinterpret_cast<uintptr_t>(d_keytab), keytab_len, d_req_stream && d_start && d_len, nreq,
                              max_len, reinterpret_cast<uintptr_t>(d_content), content_stride,
                              d_content_len && d_status && d_used && d_vouch, flags,
                              reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &g, &lay);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    const uint8_t *ftab = static_cast<const uint8_t *>(d_ftable);
    const gread::TableLayout tl(finfo->nstreams, finfo->nentries);

    GreadLaunch G{};
    G.recs = reinterpret_cast<const qread::StreamRec *>(d_table);
    G.frecs = reinterpret_cast<const gread::FrameRec *>(ftab + tl.recs);
    G.ent = reinterpret_cast<const uint64_t *>(ftab + tl.entries);
    G.key_status = nullptr;
    if (g.keyed)
        G.key_status = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(d_keytab) +
                                                          kread::TableLayout(info->nstreams).status);
    G.shape = gread::shape_of(*info, *finfo, max_len, g);
    G.req_stream = d_req_stream; G.start = d_start; G.len = d_len;
    G.q_stream = reinterpret_cast<uint32_t *>(scr + lay.q_stream);
    G.q_start = reinterpret_cast<uint64_t *>(scr + lay.q_start);
    G.q_len = reinterpret_cast<uint64_t *>(scr + lay.q_len);
    G.bad = reinterpret_cast<uint32_t *>(scr + lay.bad);
    G.stage = scr + lay.stage;
    G.stage_stride = g.stage_stride;
    G.nreq = uint32_t(nreq);
    G.content = d_content; G.stride = content_stride;
    G.content_len = d_content_len;
    G.status = d_status; G.used = d_used; G.vouch = d_vouch;
    CHIP_HIP(gread_rewrite_launch(G, s));
    // the planned read of the frame-stream requests into the staging slots, in the front part of the scratch
    const QreadCall inner{d_table, info, G.q_stream, G.q_start, G.q_len, nreq, g.inner_len, scr + lay.stage,
                          g.stage_stride, reinterpret_cast<uint64_t *>(scr + lay.q_clen), d_status, d_used, d_vouch,
                          flags, d_scratch, lay.inner_len, stream};
    st = g.keyed ? read_plain_planned(KreadCall{inner, d_keytab, keytab_len}) : read_planned(inner, true);
    if (st != CHIP_OK) return st;
    CHIP_HIP(gread_block_launch(G, s));
    CHIP_HIP(gread_finish_launch(G, s));
    return CHIP_OK;
}

}  // extern "C"
