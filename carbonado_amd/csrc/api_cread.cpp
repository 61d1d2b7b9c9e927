// api_cread.cpp — the plaintext ranged reads of include/carbonado_hip_cread.h.
// The checks, the scratch layout and the table of the keystream call are host
// code in cread_plan.hpp; this file uploads the table (through a pinned copy
// that a host function wipes behind the upload), enqueues the kernels of
// cread_kernels.hip and, last, the memset that zeroes the key region.  The
// stream keys and the read run the vouched read of api_vread.cpp in front.
#include "api_cread.hpp"
#include "api_vread.hpp"
#include "cread_kernels.hpp"
#include "key_upload.hpp"

using namespace chip;
using namespace chip::api;

namespace chip {
namespace api {

int ctr_enqueue(cread::Plan &p, uint8_t *d_buf, const uint32_t *d_gate, uint32_t *d_status, uint32_t *d_used,
                uint32_t *d_vouch, void *d_scratch, void *stream) {
    if (p.work == 0) {  // nothing has bytes: no key is used and none is uploaded
        host::secure_wipe(p.table.data(), p.table.size());
        return CHIP_OK;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    CHIP_HIP(upload_key_table(p.table, scr, s));
    CtrLaunch L{};
    L.items = reinterpret_cast<const cread::Item *>(scr + p.lay.items);
    L.rawkeys = scr + p.lay.keys;
    L.km = reinterpret_cast<cread::CtrKey *>(scr + p.lay.km);
    L.nitems = uint32_t(p.nitems);
    L.keys_used = p.keys_used;
    L.work = uint32_t(p.work);
    L.buf = d_buf;
    L.gate = d_gate;
    L.status = d_status;
    L.used = d_used;
    L.vouch = d_vouch;
    hipError_t e = ctr_setup_launch(L, s);
    if (e == hipSuccess) e = ctr_range_launch(L, s);
    // the key region goes whatever became of the launches
    const hipError_t w = hipMemsetAsync(scr + p.lay.wipe_from(), 0, p.lay.wipe_len(), s);
    CHIP_HIP(e);
    CHIP_HIP(w);
    return CHIP_OK;
}

}  // namespace api
}  // namespace chip

namespace {

// f(o) for every stream on the stage pool's threads and the caller
void for_streams(uint64_t count, const std::function<void(uint64_t)> &f) {
    const int parts = int(std::min<uint64_t>(count, 64));
    host::par_for(parts, [&](int i) {
        for (uint64_t o = uint64_t(i); o < count; o += uint64_t(parts)) f(o);
    });
}

// Scratch of chipc_stream_keys_dev: [header slots, 96 B each | status, used and
// vouch words | the vouched read's scratch].  The slots and the status words
// are one copy back.
struct KeysLayout {
    uint64_t hdrs = 0, status = 0, used = 0, vouch = 0, vread = 0, total = 0;
    explicit KeysLayout(uint64_t ns) {
        status = cread::up16(ns * cread::HDR_PITCH);
        used = status + cread::up16(ns * 4);
        vouch = used + cread::up16(ns * 4);
        vread = vouch + cread::up16(ns * 4);
        total = vread + vread::scratch_len(ns, ns);  // 81 bytes from 0 lie in one segment
    }
};

// Scratch of chipc_read_ranges_dev: [the vouched read's | the keystream call's].
uint64_t read_ctr_off(uint64_t nreq, uint64_t nseg) { return cread::up16(vread::scratch_len(nreq, nseg)); }

}  // namespace

extern "C" {

int chipc_abi_version(void) { return CHIPC_ABI_VERSION; }

uint64_t chipc_ctr_scratch_len(uint64_t nkeys, uint64_t nitems) { return cread::scratch_len(nkeys, nitems); }

int chipc_ctr_ranges_dev(const uint8_t *keys, const uint8_t *ivs, uint64_t nkeys, const uint32_t *item_key,
                         const uint64_t *pos, const uint64_t *n, uint64_t nitems, uint8_t *d_buf,
                         const uint64_t *buf_off, const uint32_t *d_gate, void *d_scratch, uint64_t scratch_len,
                         void *stream) {
    if (nitems == 0) return CHIP_OK;
    cread::Plan p;
    int st = cread::plan_ctr(keys, ivs, nkeys, item_key, pos, n, nitems, reinterpret_cast<uintptr_t>(d_buf), buf_off,
                             reinterpret_cast<uintptr_t>(d_scratch), scratch_len, nullptr, &p);
    if (st == CHIP_OK) st = use_device();
    if (st != CHIP_OK) {
        host::secure_wipe(p.table.data(), p.table.size());
        return st;
    }
    return ctr_enqueue(p, d_buf, d_gate, nullptr, nullptr, nullptr, d_scratch, stream);
}

uint64_t chipc_stream_keys_scratch_len(uint64_t nstreams) {
    if (nstreams >= (uint64_t(1) << 31)) return 0;
    return KeysLayout(nstreams).total;
}

int chipc_stream_keys_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_streams, const uint64_t *in_off,
                          const uint64_t *in_len, const uint8_t *d_hash, const uint32_t *padding,
                          const uint32_t *chunk_len, uint64_t nstreams, uint8_t *keys_out, uint8_t *ivs_out,
                          uint32_t *key_status, void *d_scratch, uint64_t scratch_len, void *stream) {
    if (nstreams == 0) return CHIP_OK;
    if (!secret_key || !keys_out || !ivs_out || !key_status || !d_scratch || !padding || !chunk_len ||
        nstreams >= (uint64_t(1) << 31))
        return CHIP_ERR_INVALID_ARG;
    const KeysLayout lay(nstreams);
    // one request per stream: envelope bytes [0, 81), or nothing of an object too short to be an envelope
    std::vector<uint32_t> req_stream(nstreams);
    std::vector<uint64_t> start(nstreams, 0), len(nstreams), coff(nstreams), clen(nstreams);
    std::vector<uint8_t> shorter(nstreams, 0);
    for (uint64_t s = 0; s < nstreams; ++s) {
        const uint64_t C = read::shard_len_alone(chunk_len[s]);
        shorter[s] = C && padding[s] <= read::K * C && read::K * C - padding[s] < cread::ENV_OVERHEAD;
        req_stream[s] = uint32_t(s);
        len[s] = shorter[s] ? 0 : cread::HDR_LEN;
        coff[s] = s * cread::HDR_PITCH;
    }
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    vread::Plan vp;
    int st = vread::plan_vread(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len,
                               reinterpret_cast<uintptr_t>(d_hash), padding, chunk_len, nstreams, req_stream.data(),
                               start.data(), len.data(), nstreams, reinterpret_cast<uintptr_t>(scr), coff.data(),
                               clen.data(), true, CHIPV_STRICT, reinterpret_cast<uintptr_t>(scr + lay.vread), ~0ull,
                               &vp);
    if (st == CHIP_ERR_INVALID_ARG || scratch_len < lay.total) return CHIP_ERR_INVALID_ARG;
    if (st != CHIP_OK) return st;
    uint8_t pub[65];
    if (sk_len != 32 || host::ecies_public_key(secret_key, pub) != CHIP_OK) return CHIP_ERR_ECIES;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t *d_status = reinterpret_cast<uint32_t *>(scr + lay.status);
    st = vread_enqueue(vp, d_status, reinterpret_cast<uint32_t *>(scr + lay.used),
                       reinterpret_cast<uint32_t *>(scr + lay.vouch), CHIPV_STRICT, scr + lay.vread, stream);
    if (st != CHIP_OK) return st;
    // the header bytes and the status words in one copy: the keys depend on them, so the call waits here
    std::vector<uint8_t> back(lay.status + nstreams * 4);
    CHIP_HIP(d2h(c->stage, back.data(), scr, back.size(), s));
    for_streams(nstreams, [&](uint64_t o) {
        const uint8_t *h = back.data() + o * cread::HDR_PITCH;
        uint32_t status;
        std::memcpy(&status, back.data() + lay.status + 4 * o, 4);
        uint8_t key[32];
        if (shorter[o]) status = CHIP_ERR_ECIES;
        else if (status == 0 && host::ecies_derive_key(secret_key, sk_len, h, key) != CHIP_OK)
            status = CHIP_ERR_ECIES;  // an ephemeral key that does not parse
        if (status == 0) {
            std::memcpy(keys_out + 32 * o, key, 32);
            std::memcpy(ivs_out + 16 * o, h + 65, 16);
        } else {
            std::memset(keys_out + 32 * o, 0, 32);
            std::memset(ivs_out + 16 * o, 0, 16);
        }
        key_status[o] = status;
        host::secure_wipe(key, sizeof key);
    });
    return CHIP_OK;
}

int chipc_read_layout(const uint32_t *chunk_len, const uint32_t *padding, uint64_t nstreams, const uint32_t *req_stream,
                      const uint64_t *start, const uint64_t *len, uint64_t nreq, uint64_t align, uint64_t *content_off,
                      uint64_t *content_len, uint64_t *content_total, uint64_t *nseg) {
    std::vector<uint64_t> sh;
    if (nreq && start) sh = cread::shifted(start, nreq);
    return read::layout(chunk_len, padding, nstreams, req_stream, nreq && start ? sh.data() : start, len, nreq, align,
                        content_off, content_len, content_total, nseg);
}

uint64_t chipc_read_scratch_len(uint64_t nreq, uint64_t nseg, uint64_t nstreams) {
    const uint64_t c = cread::scratch_len(nstreams, nreq);
    if (nreq && !c) return 0;
    return read_ctr_off(nreq, nseg) + c;
}

int chipc_read_ranges_dev(const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status, const uint8_t *d_streams,
                          const uint64_t *in_off, const uint64_t *in_len, const uint8_t *d_hash, const uint32_t *padding,
                          const uint32_t *chunk_len, uint64_t nstreams, const uint32_t *req_stream, const uint64_t *start,
                          const uint64_t *len, uint64_t nreq, uint8_t *d_content, const uint64_t *content_off,
                          uint64_t *content_len, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch, uint32_t flags,
                          void *d_scratch, uint64_t scratch_len, void *stream) {
    if (nreq == 0) return CHIP_OK;
    if (!keys || !ivs) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> sh;
    if (start && nreq < cread::MAX_ITEMS) sh = cread::shifted(start, nreq);  // (the plan refuses more before it reads one)
    const bool results = d_status && d_used && d_vouch;
    const auto plan = [&](const uint64_t *lens, uint64_t *clen, vread::Plan *vp) {
        return vread::plan_vread(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len,
                                 reinterpret_cast<uintptr_t>(d_hash), padding, chunk_len, nstreams, req_stream,
                                 start ? sh.data() : nullptr, lens, nreq, reinterpret_cast<uintptr_t>(d_content),
                                 content_off, clen, results, flags, reinterpret_cast<uintptr_t>(d_scratch), ~0ull, vp);
    };
    vread::Plan vp;
    const int vst = plan(len, content_len, &vp);
    if (vst == CHIP_ERR_INVALID_ARG) return vst;
    // the keystream over the same ranges; a request whose stream has no key is killed: zeros, its key's status
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    const uint64_t ctr_off = read_ctr_off(nreq, vp.rd.nseg);
    if (scratch_len < ctr_off) return CHIP_ERR_INVALID_ARG;
    std::vector<uint32_t> kill(nreq, 0);
    bool killed = false;
    for (uint64_t r = 0; key_status && r < nreq; ++r) {
        kill[r] = key_status[req_stream[r]];
        killed |= kill[r] != 0;
    }
    cread::Plan cp;
    int st = cread::plan_ctr(keys, ivs, nstreams, req_stream, start, content_len, nreq,
                             reinterpret_cast<uintptr_t>(d_content), content_off,
                             reinterpret_cast<uintptr_t>(scr + ctr_off), scratch_len - ctr_off, kill.data(), &cp);
    if (st == CHIP_OK) st = vst;
    if (st == CHIP_OK && killed) {  // the killed requests do no work in the vouched read either: planned again as empty
        std::vector<uint64_t> lens(len, len + nreq), clen(nreq);
        for (uint64_t r = 0; r < nreq; ++r)
            if (kill[r]) lens[r] = 0;
        vp = vread::Plan();
        st = plan(lens.data(), clen.data(), &vp);
    }
    if (st == CHIP_OK) st = use_device();
    if (st == CHIP_OK) st = vread_enqueue(vp, d_status, d_used, d_vouch, flags, d_scratch, stream);
    if (st != CHIP_OK) {
        host::secure_wipe(cp.table.data(), cp.table.size());
        return st;
    }
    return ctr_enqueue(cp, d_content, d_status, d_status, d_used, d_vouch, scr + ctr_off, stream);
}

}  // extern "C"
