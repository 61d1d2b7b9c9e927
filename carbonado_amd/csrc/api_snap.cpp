// api_snap.cpp — the snappy calls of include/carbonado_hip_snap.h over
// device-resident objects.  The checks, the scratch layouts and the tables are
// host code in snap_plan.hpp; this file uploads the table into the caller's
// scratch, enqueues the kernels of snap_kernels.hip behind it, and glues the
// one-call forms to the ragged and Ecies calls.
#include "api_common.hpp"
#include "ragged_plan.hpp"
#include "snap_kernels.hpp"
#include "snap_plan.hpp"

#include "../../include/carbonado_hip_ecies.h"
#include "../../include/carbonado_hip_ext.h"
#include "../../include/carbonado_hip_snap.h"

using namespace chip;
using namespace chip::api;

namespace {

uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

int snap_run(snap::CPlan &p, const uint8_t *d_in, uint8_t *d_out, uint64_t *d_out_len, void *d_scratch, void *stream) {
    int st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    CHIP_HIP(h2d(c->stage, scr, p.table.data(), p.table.size(), s));
    SnapLaunch L{};
    L.objs = reinterpret_cast<const snap::CObj *>(scr + p.lay.objs);
    L.blks = reinterpret_cast<const snap::CBlk *>(scr + p.lay.blks);
    L.meta = reinterpret_cast<snap::CMeta *>(scr + p.lay.meta);
    L.slots = scr + p.lay.slots;
    L.count = uint32_t(p.count);
    L.blocks = uint32_t(p.blocks);
    L.in = d_in;
    L.out = d_out;
    L.out_len = d_out_len;
    CHIP_HIP(snap_block_launch(L, s));
    CHIP_HIP(snap_frame_launch(L, s));
    CHIP_HIP(snap_gather_launch(L, s));
    return CHIP_OK;
}

int unsnap_run(snap::UPlan &p, const uint8_t *d_in, uint8_t *d_out, uint64_t *d_out_len, uint32_t *d_status,
               void *d_scratch, void *stream, bool keep_status) {
    int st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    CHIP_HIP(h2d(c->stage, scr, p.table.data(), p.table.size(), s));
    UnsnapLaunch L{};
    L.objs = reinterpret_cast<const snap::UObj *>(scr + p.lay.objs);
    L.slot_obj = reinterpret_cast<const uint32_t *>(scr + p.lay.slot_obj);
    L.desc = reinterpret_cast<snap::UDesc *>(scr + p.lay.desc);
    L.bad = reinterpret_cast<uint32_t *>(scr + p.lay.bad);
    L.state = reinterpret_cast<snap::UState *>(scr + p.lay.state);
    L.count = uint32_t(p.count);
    L.slots = uint32_t(p.slots);
    L.in = d_in;
    L.out = d_out;
    L.out_len = d_out_len;
    L.status = d_status;
    L.keep_status = keep_status;
    CHIP_HIP(unsnap_walk_launch(L, s));
    CHIP_HIP(unsnap_block_launch(L, s));
    CHIP_HIP(unsnap_crc_launch(L, s));
    CHIP_HIP(unsnap_finish_launch(L, s));
    return CHIP_OK;
}

// Scratch of the one-call forms: rows (row o of up16(bound[o]) bytes) | compressed lengths (encode) |
// snap scratch | the scratch of the ragged or Ecies call.
struct Regions {
    std::vector<uint64_t> row_off;
    uint64_t lens = 0, snap = 0, inner = 0, total = 0;
};

bool encode_regions(uint8_t format, const uint64_t *n, uint64_t count, std::vector<uint64_t> *frame_max,
                    std::vector<uint64_t> *stage_max, Regions *r) {
    if (!snap::snap_format(format) || !n || count == 0 || count >= snap::MAX_COUNT) return false;
    frame_max->resize(count);
    stage_max->resize(count);
    r->row_off.resize(count);
    uint64_t at = 0;
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > snap::MAX_STAGE) return false;
        (*frame_max)[o] = snap::max_len(n[o]);
        (*stage_max)[o] = snap::worst_stage_len(format, n[o]);
        if ((*stage_max)[o] > snap::MAX_STAGE) return false;
        r->row_off[o] = at;
        at += snap::up16((*frame_max)[o]);
    }
    const uint64_t sn = snap::snap_scratch_len(n, count);
    if (!sn) return false;
    uint64_t in;
    if (format & CHIP_FORMAT_ECIES) {
        in = chipe_encode_scratch_len(format & 13, frame_max->data(), count);
        if (!in) return false;
    } else {
        in = chipx_ragged_scratch_len(format & 12, frame_max->data(), count, 0);
    }
    r->lens = at;
    r->snap = r->lens + snap::up16(8 * count);
    r->inner = r->snap + sn;
    r->total = snap::up16(r->inner + in);
    return true;
}

bool decode_regions(uint8_t format, const uint64_t *in_len, const uint64_t *out_cap, uint64_t count, Regions *r) {
    if (!snap::snap_format(format) || !in_len || !out_cap || count == 0 || count >= snap::MAX_COUNT) return false;
    r->row_off.resize(count);
    uint64_t at = 0;
    for (uint64_t o = 0; o < count; ++o) {
        if (in_len[o] > 4 * snap::MAX_STAGE) return false;
        r->row_off[o] = at;  // a stream is longer than what it decodes to
        at += snap::up16(in_len[o]);
    }
    const uint64_t un = snap::unsnap_scratch_len(in_len, out_cap, count);
    if (!un) return false;
    uint64_t in;
    if (format & CHIP_FORMAT_ECIES) {
        in = chipe_decode_scratch_len(format & 13, in_len, count);
        if (!in) return false;
    } else {
        in = chipx_ragged_scratch_len(format & 12, in_len, count, 1);
    }
    r->lens = at;
    r->snap = at;
    r->inner = r->snap + un;
    r->total = snap::up16(r->inner + in);
    return true;
}

}  // namespace

extern "C" {

int chips_abi_version(void) { return CHIPS_ABI_VERSION; }

uint64_t chips_snap_scratch_len(const uint64_t *n, uint64_t count) { return snap::snap_scratch_len(n, count); }

uint64_t chips_unsnap_scratch_len(const uint64_t *in_len, const uint64_t *out_cap, uint64_t count) {
    return snap::unsnap_scratch_len(in_len, out_cap, count);
}

int chips_snap_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                          uint8_t *d_out, const uint64_t *out_off, uint64_t *d_out_len, void *d_scratch,
                          uint64_t scratch_len, void *stream) {
    if (count == 0) return CHIP_OK;
    snap::CPlan p;
    int st = snap::plan_snap(addr(d_in), in_off, n, count, addr(d_out), out_off, d_out_len != nullptr,
                             addr(d_scratch), scratch_len, &p);
    if (st != CHIP_OK) return st;
    return snap_run(p, d_in, d_out, d_out_len, d_scratch, stream);
}

int chips_unsnap_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                            uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len,
                            uint32_t *d_status, void *d_scratch, uint64_t scratch_len, void *stream) {
    if (count == 0) return CHIP_OK;
    snap::UPlan p;
    int st = snap::plan_unsnap(addr(d_in), in_off, in_len, count, addr(d_out), out_off, out_cap,
                               d_out_len != nullptr, d_status != nullptr, addr(d_scratch), scratch_len, &p);
    if (st != CHIP_OK) return st;
    return unsnap_run(p, d_in, d_out, d_out_len, d_status, d_scratch, stream, false);
}

// ---- formats 6, 7, 10, 11, 14, 15 ---------------------------------------------------
int chips_encode_layout(uint8_t format, const uint64_t *n, uint64_t count, uint64_t align, uint64_t stream_offset,
                        uint64_t *out_off, uint64_t *out_cap, uint64_t *total) {
    if (!snap::snap_format(format) || !total || (count && (!n || !out_off || !out_cap)) || count >= snap::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> worst(count);
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > snap::MAX_STAGE) return CHIP_ERR_INVALID_ARG;
        worst[o] = snap::worst_stage_len(format, n[o]);
        if (worst[o] > snap::MAX_STAGE) return CHIP_ERR_INVALID_ARG;
    }
    return ragged::layout(format & 12, worst.data(), count, align, stream_offset, out_off, out_cap, total);
}

uint64_t chips_encode_scratch_len(uint8_t format, const uint64_t *n, uint64_t count) {
    std::vector<uint64_t> fm, sm;
    Regions r;
    return encode_regions(format, n, count, &fm, &sm, &r) ? r.total : 0;
}

uint64_t chips_decode_scratch_len(uint8_t format, const uint64_t *in_len, const uint64_t *out_cap, uint64_t count) {
    Regions r;
    return decode_regions(format, in_len, out_cap, count, &r) ? r.total : 0;
}

int chips_encode_ragged_dev(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                            const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                            uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, uint8_t *d_hash,
                            chip_encode_info *info, void *d_scratch, void *stream) {
    if (!snap::snap_format(format)) return CHIP_ERR_INVALID_ARG;
    if (count == 0) return CHIP_OK;
    const bool ecies = format & CHIP_FORMAT_ECIES;
    if (!in_off || !n || !out_off || !out_len || !d_out || !d_hash || !d_scratch || (ecies && !pubkey) ||
        misaligned16(d_scratch) || count >= snap::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> frame_max, stage_max;
    Regions r;
    if (!encode_regions(format, n, count, &frame_max, &stage_max, &r)) return CHIP_ERR_INVALID_ARG;
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    uint64_t *d_lens = reinterpret_cast<uint64_t *>(scr + r.lens);
    snap::CPlan sp;
    int st = snap::plan_snap(addr(d_in), in_off, n, count, addr(scr), r.row_off.data(), true, addr(scr + r.snap),
                             ~uint64_t(0), &sp);
    if (st != CHIP_OK) return st;
    {  // the zfec / bao half's own checks over the worst-case lengths, before anything is enqueued
        ragged::Plan rp;
        std::vector<uint64_t> worst_out(count);
        st = ragged::plan_encode(format & 12, addr(scr), r.row_off.data(), stage_max.data(), count, addr(d_out), out_off,
                                 worst_out.data(), &rp);
        if (st != CHIP_OK) return st;
    }
    if (ecies) {
        uint8_t peer[65];
        st = host::ecies_peer(pubkey, pubkey_len, peer);
        if (st != CHIP_OK) return st;
    }
    st = snap_run(sp, d_in, scr, d_lens, scr + r.snap, stream);
    if (st != CHIP_OK) return st;
    // the compressed lengths: the layout of everything after depends on them, so the call waits here
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    std::vector<uint64_t> clen(count);
    CHIP_HIP(d2h(c->stage, clen.data(), d_lens, 8 * count, static_cast<hipStream_t>(stream)));
    if (ecies)
        st = chipe_encode_ragged_dev(format & 13, pubkey, pubkey_len, inject, scr, r.row_off.data(), clen.data(), count,
                                     d_out, out_off, out_len, d_hash, nullptr, scr + r.inner, stream);
    else
        st = chipx_encode_ragged_dev(format & 12, scr, r.row_off.data(), clen.data(), count, d_out, out_off, out_len,
                                     d_hash, nullptr, scr + r.inner, stream);
    if (st != CHIP_OK) return st;
    for (uint64_t o = 0; info && o < count; ++o) {  // EncodeInfo of encode() at `format` (encoding.rs:86-171)
        const uint64_t env = ecies ? clen[o] + snap::ENV_OVERHEAD : 0;
        uint64_t zlen, fl;
        st = encode_info_for(format, n[o], ecies ? env : clen[o], clen[o], env, &info[o], &zlen, &fl);
        if (st != CHIP_OK) return st;
    }
    return CHIP_OK;
}

int chips_decode_ragged_dev(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                            const uint64_t *in_off, const uint64_t *in_len, uint64_t count, const uint8_t *d_hash,
                            const uint32_t *padding, uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap,
                            uint64_t *d_out_len, uint32_t *d_status, void *d_scratch, void *stream) {
    if (!snap::snap_format(format)) return CHIP_ERR_INVALID_ARG;
    if (count == 0) return CHIP_OK;
    const bool ecies = format & CHIP_FORMAT_ECIES;
    if (!d_in || !in_off || !in_len || !out_off || !out_cap || !d_out_len || !d_status || !d_scratch ||
        (ecies && !secret_key) || misaligned16(d_scratch) || count >= snap::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    Regions r;
    if (!decode_regions(format, in_len, out_cap, count, &r)) return CHIP_ERR_INVALID_ARG;
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    const uint8_t f12 = format & 12;
    std::vector<uint64_t> frame_len(count), got(count);
    snap::UPlan up;
    {  // both halves' checks, before anything is enqueued
        ragged::Plan rp;
        int st = ragged::plan_decode(f12, addr(d_in), in_off, in_len, count, padding, addr(scr), r.row_off.data(),
                                     frame_len.data(), &rp);
        if (st != CHIP_OK) return st;
        if ((f12 & CHIP_FORMAT_BAO) && !d_hash) return CHIP_ERR_HASH_DECODE;
        if (ecies)  // what the row holds is an envelope
            for (uint64_t o = 0; o < count; ++o)
                frame_len[o] = frame_len[o] >= snap::ENV_OVERHEAD ? frame_len[o] - snap::ENV_OVERHEAD : 0;
        st = snap::plan_unsnap(addr(scr), r.row_off.data(), frame_len.data(), count, addr(d_out), out_off, out_cap, true,
                               true, addr(scr + r.snap), ~uint64_t(0), &up);
        if (st != CHIP_OK) return st;
    }
    int st;
    if (ecies) {
        // the envelopes into a region of their own inside the Ecies call's scratch; the frames into the rows
        st = chipe_decode_ragged_dev(format & 13, secret_key, sk_len, d_in, in_off, in_len, count, d_hash, padding, scr,
                                     r.row_off.data(), got.data(), d_status, scr + r.inner, stream);
    } else {
        st = chipx_decode_ragged_dev(f12, d_in, in_off, in_len, count, d_hash, padding, scr, r.row_off.data(),
                                     got.data(), d_status, scr + r.inner, stream);
    }
    if (st != CHIP_OK) return st;
    return unsnap_run(up, scr, d_out, d_out_len, d_status, scr + r.snap, stream, true);
}

}  // extern "C"
