// api_kread.cpp — the device-planned plaintext reads of level-13 objects of
// include/carbonado_hip_kread.h.  chipk_key_table_dev is the one key setup of a
// set of resident streams: the key_status words and the raw records uploaded
// through the pinned copy (key_upload.hpp), KC's setup kernel over them, and
// KK's finish kernel, which zeroes the raw records.  A read call does O(1) host
// work (kread::plan_call) and enqueues KK's rewrite, the device-planned vouched
// read of api_qread.cpp over the rewritten requests, and KK's keystream
// kernel.  Kernels only: no upload, no memset, no synchronisation, no
// allocation after the thread's first call.  The read's enqueue is
// read_plain_planned, declared in api_kread.hpp: api_gread.cpp runs it over
// requests its own kernel rewrote.
#include "api_kread.hpp"
#include "cread_kernels.hpp"
#include "key_upload.hpp"

using namespace chip;
using namespace chip::api;

namespace chip {
namespace api {

int read_plain_planned(const KreadCall &a) {
    const void *d_table = a.q.d_table;
    const chipq_table_info *info = a.q.info;
    const void *d_keytab = a.d_keytab;
    const uint64_t keytab_len = a.keytab_len;
    const uint32_t *d_req_stream = a.q.d_req_stream;
    const uint64_t *d_start = a.q.d_start, *d_len = a.q.d_len;
    const uint64_t nreq = a.q.nreq, max_len = a.q.max_len, content_stride = a.q.content_stride;
    uint8_t *d_content = a.q.d_content;
    uint64_t *d_content_len = a.q.d_content_len;
    uint32_t *d_status = a.q.d_status, *d_used = a.q.d_used, *d_vouch = a.q.d_vouch;
    const uint32_t flags = a.q.flags;
    void *d_scratch = a.q.d_scratch;
    const uint64_t scratch_len = a.q.scratch_len;
    void *stream = a.q.stream;
    if (nreq == 0) return CHIP_OK;
    kread::Geometry g;
    kread::ScratchLayout lay;
    int st = kread::plan_call(reinterpret_cast<uintptr_t>(d_table), info, reinterpret_cast<uintptr_t>(d_keytab),
                              keytab_len, d_req_stream && d_start && d_len, nreq, max_len,
                              reinterpret_cast<uintptr_t>(d_content), content_stride,
                              d_content_len && d_status && d_used && d_vouch, flags,
                              reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &g, &lay);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    const uint8_t *tab = static_cast<const uint8_t *>(d_keytab);
    const kread::TableLayout tl(info->nstreams);

    KreadLaunch K{};
    K.recs = reinterpret_cast<const qread::StreamRec *>(d_table);
    K.shape = qread::Shape{info->nstreams, info->max_chunks, info->min_shard, max_len, g.q.S};
    K.km = reinterpret_cast<const cread::CtrKey *>(tab + tl.km);
    K.key_status = reinterpret_cast<const uint32_t *>(tab + tl.status);
    K.req_stream = d_req_stream; K.start = d_start; K.len = d_len;
    K.q_stream = reinterpret_cast<uint32_t *>(scr + lay.q_stream);
    K.q_start = reinterpret_cast<uint64_t *>(scr + lay.q_start);
    K.q_len = reinterpret_cast<uint64_t *>(scr + lay.q_len);
    K.nreq = uint32_t(nreq); K.cap = g.cap;
    K.content = d_content; K.stride = content_stride;
    K.content_len = d_content_len;
    K.status = d_status; K.used = d_used; K.vouch = d_vouch;
    CHIP_HIP(kread_rewrite_launch(K, s));
    // the vouched read of the envelope requests, in the front part of the scratch
    st = read_planned(QreadCall{d_table, info, K.q_stream, K.q_start, K.q_len, nreq, max_len, d_content,
                                content_stride, d_content_len, d_status, d_used, d_vouch, flags, d_scratch,
                                lay.q.total, stream},
                      true);
    if (st != CHIP_OK) return st;
    CHIP_HIP(kread_ctr_launch(K, s));
    return CHIP_OK;
}

}  // namespace api
}  // namespace chip

extern "C" {

int chipk_abi_version(void) { return CHIPK_ABI_VERSION; }

uint64_t chipk_key_table_len(uint64_t nstreams) { return kread::table_len(nstreams); }

int chipk_key_table_dev(const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status, uint64_t nstreams,
                        void *d_keytab, uint64_t keytab_len, void *stream) {
    if (nstreams == 0) return CHIP_OK;
    int st = kread::check_table(keys != nullptr, ivs != nullptr, reinterpret_cast<uintptr_t>(d_keytab), nstreams,
                                keytab_len);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const kread::TableLayout lay(nstreams);
    uint8_t *tab = static_cast<uint8_t *>(d_keytab);
    std::vector<uint8_t> words = kread::table_upload(keys, ivs, key_status, nstreams);
    CHIP_HIP(upload_key_table(words, tab + lay.status, s));  // wipes `words`
    CtrLaunch L{};
    L.rawkeys = tab + lay.raw;
    L.km = reinterpret_cast<cread::CtrKey *>(tab + lay.km);
    L.keys_used = uint32_t(nstreams);
    hipError_t e = ctr_setup_launch(L, s);
    // the raw records go whatever became of the setup
    const hipError_t w = kread_table_finish_launch(L.km, reinterpret_cast<const uint32_t *>(tab + lay.status),
                                                   tab + lay.raw, uint32_t(nstreams), s);
    CHIP_HIP(e);
    CHIP_HIP(w);
    return CHIP_OK;
}

int chipk_key_table_wipe_dev(void *d_keytab, uint64_t keytab_len, void *stream) {
    if (keytab_len == 0) return CHIP_OK;
    if (!d_keytab) return CHIP_ERR_INVALID_ARG;
    const int st = use_device();
    if (st != CHIP_OK) return st;
    CHIP_HIP(hipMemsetAsync(d_keytab, 0, keytab_len, static_cast<hipStream_t>(stream)));
    return CHIP_OK;
}

uint64_t chipk_read_scratch_len(const chipq_table_info *info, uint64_t nreq, uint64_t max_len) {
    return kread::scratch_len(info, nreq, max_len);
}

int chipk_read_ranges_dev(const void *d_table, const chipq_table_info *info, const void *d_keytab, uint64_t keytab_len,
                          const uint32_t *d_req_stream, const uint64_t *d_start, const uint64_t *d_len, uint64_t nreq,
                          uint64_t max_len, uint8_t *d_content, uint64_t content_stride, uint64_t *d_content_len,
                          uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch, uint32_t flags, void *d_scratch,
                          uint64_t scratch_len, void *stream) {
    return read_plain_planned(KreadCall{QreadCall{d_table, info, d_req_stream, d_start, d_len, nreq, max_len, d_content,
                                                  content_stride, d_content_len, d_status, d_used, d_vouch, flags,
                                                  d_scratch, scratch_len, stream},
                                        d_keytab, keytab_len});
}

}  // extern "C"
