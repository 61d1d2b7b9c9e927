// api_fread.cpp — the plaintext ranged reads of level-14 / level-15 streams of
// include/carbonado_hip_fread.h.  The checks, the scratch layouts and the tables
// are host code in fread_plan.hpp; this file runs the vouched read of
// api_vread.cpp and the keystream of api_cread.cpp in front of the kernels of
// fread_kernels.hip.  The index build waits twice (for the walked offsets, for
// the chain's verdicts); the index check and the read wait for nothing.
#include "api_cread.hpp"
#include "api_vread.hpp"
#include "cread_kernels.hpp"
#include "fread_kernels.hpp"
#include "fread_plan.hpp"
#include "key_upload.hpp"

using namespace chip;
using namespace chip::api;

namespace {

// entries beyond the caller's that layer 2 may hand layer 1: the header a walk stopped at, and L
constexpr uint64_t SPARE = 2;

fread::IndexLayout index_layout(uint64_t ns, uint64_t ne) { return fread::IndexLayout(ns, ne + SPARE * ns); }

// What the two index calls check of the stream arguments, in the header's order.
struct Streams {
    std::vector<fread::Geo> geo;
    std::vector<uint32_t> skip;  // key_status, or CHIP_ERR_ZFEC for a stream that does not fit
    bool truncated = false;
};

int check_streams(uint8_t format, const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status,
                  const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len, const uint32_t *padding,
                  const uint32_t *chunk_len, uint64_t ns, bool others, const void *d_scratch, Streams *out) {
    if (!fread::format_ok(format)) return CHIP_ERR_INVALID_ARG;
    if (format == 15 && (!keys || !ivs)) return CHIP_ERR_INVALID_ARG;
    if (!d_streams || !in_off || !in_len || !padding || !chunk_len || !others || !d_scratch)
        return CHIP_ERR_INVALID_ARG;
    if (ns >= fread::MAX_STREAMS) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> n;
    const int st = audit::stream_lengths(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len, ns, &n, &out->truncated);
    if (st != CHIP_OK) return st;
    if (reinterpret_cast<uintptr_t>(d_scratch) & 15u) return CHIP_ERR_INVALID_ARG;
    out->geo.resize(ns);
    out->skip.assign(ns, 0);
    for (uint64_t s = 0; s < ns; ++s) {
        out->geo[s] = fread::geo_of(n[s], chunk_len[s], padding[s], fread::shift_of(format));
        out->skip[s] = format == 15 && key_status && key_status[s] ? key_status[s] : out->geo[s].status;
    }
    return CHIP_OK;
}

// Layer 1 behind its host checks: the header reads, the keystream over them and
// the chain kernel, its three words per stream to the given device arrays.
int verify_enqueue(uint8_t format, const uint8_t *keys, const uint8_t *ivs, const uint8_t *d_streams,
                   const uint64_t *in_off, const uint64_t *in_len, const uint8_t *d_hash, const uint32_t *padding,
                   const uint32_t *chunk_len, const Streams &S, const std::vector<uint64_t> &offs,
                   const std::vector<uint32_t> &nfr, uint32_t *d_ostat, uint64_t *d_oplain, uint32_t *d_ovouch,
                   uint8_t *scr, const fread::IndexLayout &lay, void *stream) {
    const uint64_t ns = nfr.size();
    fread::VerifyPlan vp;
    fread::plan_verify(offs, nfr, S.skip, S.geo, fread::shift_of(format), &vp);
    vread::Plan rp;
    int st = vread::plan_vread(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len,
                               reinterpret_cast<uintptr_t>(d_hash), padding, chunk_len, ns, vp.req_stream.data(),
                               vp.start.data(), vp.len.data(), vp.nreq, reinterpret_cast<uintptr_t>(scr + lay.rows),
                               vp.coff.data(), vp.clen.data(), true, CHIPV_STRICT,
                               reinterpret_cast<uintptr_t>(scr + lay.vread), ~0ull, &rp);
    if (st != CHIP_OK) return st;
    cread::Plan cp;
    if (format == 15) {
        st = cread::plan_ctr(keys, ivs, ns, vp.req_stream.data(), vp.pos.data(), vp.clen.data(), vp.nreq,
                             reinterpret_cast<uintptr_t>(scr + lay.rows), vp.coff.data(),
                             reinterpret_cast<uintptr_t>(scr + lay.ctr), ~0ull, nullptr, &cp);
    }
    const auto fail = [&](int code) {
        host::secure_wipe(cp.table.data(), cp.table.size());
        return code;
    };
    if (st != CHIP_OK) return fail(st);
    st = use_device();
    if (st != CHIP_OK) return fail(st);
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return fail(st);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t *rstat = reinterpret_cast<uint32_t *>(scr + lay.rstat);
    uint32_t *rvouch = reinterpret_cast<uint32_t *>(scr + lay.rvouch);
    if (h2d(c->stage, scr + lay.vtab, vp.table.data(), vp.table.size(), s) != hipSuccess) return fail(CHIP_ERR_DEVICE);
    st = vread_enqueue(rp, rstat, reinterpret_cast<uint32_t *>(scr + lay.rused), rvouch, CHIPV_STRICT, scr + lay.vread,
                       stream);
    if (st != CHIP_OK) return fail(st);
    if (format == 15) {
        st = ctr_enqueue(cp, scr + lay.rows, rstat, nullptr, nullptr, nullptr, scr + lay.ctr, stream);
        if (st != CHIP_OK) return st;
    }
    ChainLaunch L{};
    L.streams = reinterpret_cast<const fread::VStream *>(scr + lay.vtab);
    L.off = reinterpret_cast<const uint64_t *>(scr + lay.voff);
    L.rows = scr + lay.rows;
    L.rstat = rstat;
    L.rvouch = rvouch;
    L.status = d_ostat;
    L.plain = d_oplain;
    L.vouch = d_ovouch;
    L.count = uint32_t(ns);
    CHIP_HIP(fread_chain_launch(L, s));
    return CHIP_OK;
}

}  // namespace

extern "C" {

int chipf_abi_version(void) { return CHIPF_ABI_VERSION; }

uint64_t chipf_index_scratch_len(uint64_t nstreams, uint64_t nentries) {
    if (nstreams >= fread::MAX_STREAMS || nentries >= fread::MAX_ENTRIES) return 0;
    return index_layout(nstreams, nentries).total;
}

int chipf_verify_index_dev(uint8_t format, const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status,
                           const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                           const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                           const uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *nframes,
                           uint32_t *d_index_status, uint64_t *d_plain_len, uint32_t *d_index_vouch, void *d_scratch,
                           uint64_t scratch_len, void *stream) {
    if (nstreams == 0) return CHIP_OK;
    Streams S;
    int st = check_streams(format, keys, ivs, key_status, d_streams, in_off, in_len, padding, chunk_len, nstreams,
                           frame_off && idx_off && nframes && d_index_status && d_plain_len && d_index_vouch, d_scratch,
                           &S);
    if (st != CHIP_OK) return st;
    uint64_t ne = 0;
    for (uint64_t s = 0; s < nstreams; ++s) {
        if (nframes[s] >= fread::MAX_ENTRIES || idx_off[s] > fread::MAX_RANGE) return CHIP_ERR_INVALID_ARG;
        ne += nframes[s] + 1;
        if (ne >= fread::MAX_ENTRIES) return CHIP_ERR_INVALID_ARG;
    }
    std::vector<uint64_t> offs;
    std::vector<uint32_t> nfr(nstreams);
    offs.reserve(ne);
    for (uint64_t s = 0; s < nstreams; ++s) {
        nfr[s] = uint32_t(nframes[s]);
        for (uint64_t f = 0; f <= nframes[s]; ++f) {
            const uint64_t o = frame_off[idx_off[s] + f];
            if (o > fread::MAX_RANGE) return CHIP_ERR_INVALID_ARG;
            offs.push_back(o);
        }
    }
    const fread::IndexLayout lay = index_layout(nstreams, ne);
    if (scratch_len < lay.total) return CHIP_ERR_INVALID_ARG;
    if (S.truncated) return CHIP_ERR_BAO_TRUNCATED;
    if (!d_hash) return CHIP_ERR_HASH_DECODE;
    return verify_enqueue(format, keys, ivs, d_streams, in_off, in_len, d_hash, padding, chunk_len, S, offs, nfr,
                          d_index_status, d_plain_len, d_index_vouch, static_cast<uint8_t *>(d_scratch), lay, stream);
}

int chipf_frame_index_dev(uint8_t format, const uint8_t *keys, const uint8_t *ivs, const uint32_t *key_status,
                          const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                          const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                          uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *idx_cap, uint64_t *nframes,
                          uint32_t *index_status, uint64_t *plain_len, uint32_t *index_vouch, void *d_scratch,
                          uint64_t scratch_len, void *stream) {
    if (nstreams == 0) return CHIP_OK;
    Streams S;
    int st = check_streams(format, keys, ivs, key_status, d_streams, in_off, in_len, padding, chunk_len, nstreams,
                           frame_off && idx_off && idx_cap && nframes && index_status && plain_len && index_vouch,
                           d_scratch, &S);
    if (st != CHIP_OK) return st;
    const uint64_t ns = nstreams;
    uint64_t ne = 0;
    for (uint64_t s = 0; s < ns; ++s) {
        if (idx_cap[s] >= fread::MAX_ENTRIES || idx_off[s] > fread::MAX_RANGE) return CHIP_ERR_INVALID_ARG;
        ne += idx_cap[s];
        if (ne >= fread::MAX_ENTRIES) return CHIP_ERR_INVALID_ARG;
    }
    const fread::IndexLayout lay = index_layout(ns, ne);
    if (scratch_len < lay.total) return CHIP_ERR_INVALID_ARG;
    if (S.truncated) return CHIP_ERR_BAO_TRUNCATED;
    if (!d_hash) return CHIP_ERR_HASH_DECODE;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);

    // the walk's table: its streams, and at 15 the raw keys behind them (one upload through the pinned copy)
    const bool keyed = format == 15;
    std::vector<uint8_t> table(keyed ? lay.km : ns * sizeof(fread::WStream), 0);
    std::vector<uint64_t> ent0(ns);
    uint64_t e = 0;
    for (uint64_t s = 0; s < ns; ++s) {
        fread::WStream w{};
        w.src = in_off[s];
        w.L = S.geo[s].L;
        w.ent0 = ent0[s] = e;
        w.N = S.geo[s].N;
        w.cap = uint32_t(idx_cap[s]);
        w.shift = uint32_t(fread::shift_of(format));
        w.skip = S.skip[s];
        w.key = uint32_t(s);
        std::memcpy(table.data() + s * sizeof w, &w, sizeof w);
        if (keyed && !w.skip) {
            std::memcpy(table.data() + lay.rawkeys + 48 * s, keys + 32 * s, 32);
            std::memcpy(table.data() + lay.rawkeys + 48 * s + 32, ivs + 16 * s, 16);
        }
        e += idx_cap[s];
    }
    if (keyed) {
        CHIP_HIP(upload_key_table(table, scr, hs));
        CtrLaunch K{};
        K.rawkeys = scr + lay.rawkeys;
        K.km = reinterpret_cast<cread::CtrKey *>(scr + lay.km);
        K.keys_used = uint32_t(ns);
        const hipError_t e1 = ctr_setup_launch(K, hs);
        if (e1 != hipSuccess) {
            (void)hipMemsetAsync(scr + lay.wipe_from(), 0, lay.wipe_len(), hs);
            CHIP_HIP(e1);
        }
    } else {
        CHIP_HIP(h2d(c->stage, scr, table.data(), table.size(), hs));
    }
    WalkLaunch W{};
    W.streams = reinterpret_cast<const fread::WStream *>(scr);
    W.km = reinterpret_cast<const cread::CtrKey *>(scr + lay.km);
    W.in = d_streams;
    W.out = reinterpret_cast<fread::WalkOut *>(scr + lay.wout);
    W.off = reinterpret_cast<uint64_t *>(scr + lay.woff);
    W.count = uint32_t(ns);
    const hipError_t e2 = fread_walk_launch(W, hs);
    // the key region goes whatever became of the launch
    const hipError_t e3 = keyed ? hipMemsetAsync(scr + lay.wipe_from(), 0, lay.wipe_len(), hs) : hipSuccess;
    CHIP_HIP(e2);
    CHIP_HIP(e3);
    // what the walk found and the offsets in one copy: layer 1 depends on them, so the call waits here
    std::vector<uint8_t> back(lay.woff - lay.wout + ne * 8);
    CHIP_HIP(d2h(c->stage, back.data(), scr + lay.wout, back.size(), hs));
    const fread::WalkOut *wo = reinterpret_cast<const fread::WalkOut *>(back.data());
    const uint64_t *woff = reinterpret_cast<const uint64_t *>(back.data() + (lay.woff - lay.wout));

    std::vector<uint64_t> offs;
    std::vector<uint32_t> nfr(ns);
    Streams V = S;  // layer 1's view: a stream whose capacity is too small is skipped with that status
    for (uint64_t s = 0; s < ns; ++s) {
        const fread::WalkOut &o = wo[s];
        const uint64_t *mine = woff + ent0[s];
        const uint64_t have = std::min<uint64_t>(o.nframes, idx_cap[s]);
        nframes[s] = o.nframes;
        if (S.skip[s] || o.status == fread::ST_TOO_SMALL) {
            V.skip[s] = S.skip[s] ? S.skip[s] : o.status;
            nfr[s] = 0;
            offs.push_back(0);
            if (!S.skip[s])
                for (uint64_t f = 0; f < have; ++f) frame_off[idx_off[s] + f] = mine[f];
            continue;
        }
        for (uint64_t f = 0; f < have; ++f) {
            frame_off[idx_off[s] + f] = mine[f];
            offs.push_back(mine[f]);
        }
        if (o.status == fread::ST_OK) {  // have == nframes < cap: the last entry fits
            frame_off[idx_off[s] + have] = S.geo[s].L;
            offs.push_back(S.geo[s].L);
            nfr[s] = uint32_t(have);
        } else {  // the header the walk stopped at is read too: its vouch word tells damage from a bad stream
            offs.push_back(o.bad_pos);
            offs.push_back(S.geo[s].L);
            nfr[s] = uint32_t(have + 1);
        }
    }
    st = verify_enqueue(format, keys, ivs, d_streams, in_off, in_len, d_hash, padding, chunk_len, V, offs, nfr,
                        reinterpret_cast<uint32_t *>(scr + lay.ostat), reinterpret_cast<uint64_t *>(scr + lay.oplain),
                        reinterpret_cast<uint32_t *>(scr + lay.ovouch), scr, lay, stream);
    if (st != CHIP_OK) return st;
    std::vector<uint8_t> words(lay.out_len);
    CHIP_HIP(d2h(c->stage, words.data(), scr + lay.ostat, words.size(), hs));
    const uint32_t *ostat = reinterpret_cast<const uint32_t *>(words.data());
    const uint32_t *ovouch = reinterpret_cast<const uint32_t *>(words.data() + (lay.ovouch - lay.ostat));
    const uint64_t *oplain = reinterpret_cast<const uint64_t *>(words.data() + (lay.oplain - lay.ostat));
    for (uint64_t s = 0; s < ns; ++s) {
        uint32_t status = ostat[s];
        const uint32_t walked = wo[s].status;
        if (!S.skip[s] && (walked == fread::ST_UNSUPPORTED || walked == fread::ST_SNAP) && status != fread::ST_HASH &&
            status != fread::ST_ZFEC)
            status = walked;
        index_status[s] = status;
        index_vouch[s] = ovouch[s];
        plain_len[s] = status == 0 ? oplain[s] : 0;
    }
    return CHIP_OK;
}

int chipf_read_layout(uint8_t format, const uint32_t *chunk_len, const uint32_t *padding, const uint32_t *index_status,
                      const uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *nframes,
                      const uint64_t *plain_len, uint64_t nstreams,
                      const uint32_t *req_stream, const uint64_t *start, const uint64_t *len, uint64_t nreq,
                      uint64_t align, uint64_t *content_off, uint64_t *content_len, uint64_t *content_total,
                      uint64_t *nseg, uint64_t *stage_total, uint64_t *vseg) {
    if (!fread::format_ok(format) || align == 0 || align % 16) return CHIP_ERR_INVALID_ARG;
    if (nreq && (!chunk_len || !padding || !frame_off || !idx_off || !nframes || !plain_len || !req_stream || !start ||
                 !len))
        return CHIP_ERR_INVALID_ARG;
    fread::ReadPlan p;
    if (nreq) {
        const int st = fread::check_reads(format, 0, chunk_len, padding, frame_off, idx_off, nframes, plain_len,
                                          index_status, nstreams, req_stream, start, len, nreq);
        if (st != CHIP_OK) return st;
        fread::plan_ranges(chunk_len, padding, frame_off, idx_off, plain_len, index_status, fread::shift_of(format),
                           req_stream, start, len, nreq, &p);
    }
    fread::layout_content(p, align, content_off, content_len, content_total);
    if (nseg) *nseg = p.nseg;
    if (stage_total) *stage_total = p.stage_total;
    if (vseg) *vseg = p.vseg;
    return CHIP_OK;
}

uint64_t chipf_read_scratch_len(uint64_t nreq, uint64_t nseg, uint64_t stage_total, uint64_t vseg, uint64_t nstreams) {
    return fread::read_scratch_len(nreq, nseg, stage_total, vseg, nstreams);
}

int chipf_read_ranges_dev(uint8_t format, const uint8_t *keys, const uint8_t *ivs, const uint32_t *index_status,
                          const uint64_t *frame_off, const uint64_t *idx_off, const uint64_t *nframes,
                          const uint64_t *plain_len, const uint8_t *d_streams, const uint64_t *in_off,
                          const uint64_t *in_len, const uint8_t *d_hash, const uint32_t *padding,
                          const uint32_t *chunk_len, uint64_t nstreams, const uint32_t *req_stream,
                          const uint64_t *start, const uint64_t *len, uint64_t nreq, uint8_t *d_content,
                          const uint64_t *content_off, uint64_t *content_len, uint32_t *d_status, uint32_t *d_used,
                          uint32_t *d_vouch, uint32_t flags, void *d_scratch, uint64_t scratch_len, void *stream) {
    if (nreq == 0) return CHIP_OK;
    if ((format == 15 && (!keys || !ivs)) || !frame_off || !idx_off || !nframes || !plain_len)
        return CHIP_ERR_INVALID_ARG;
    if (!d_streams || !in_off || !in_len || !padding || !chunk_len || !req_stream || !start || !len || !content_off ||
        !content_len || !d_status || !d_used || !d_vouch || !d_scratch)
        return CHIP_ERR_INVALID_ARG;
    int st = fread::check_reads(format, flags, chunk_len, padding, frame_off, idx_off, nframes, plain_len, index_status,
                                nstreams, req_stream, start, len, nreq);
    if (st != CHIP_OK) return st;
    fread::ReadPlan p;
    fread::plan_ranges(chunk_len, padding, frame_off, idx_off, plain_len, index_status, fread::shift_of(format),
                       req_stream, start, len, nreq, &p);
    fread::layout_content(p, 16, nullptr, content_len, nullptr);
    bool any = false;
    for (uint64_t r = 0; r < nreq; ++r) {
        if (content_off[r] > fread::MAX_RANGE) return CHIP_ERR_INVALID_ARG;
        any |= content_len[r] != 0;
    }
    if (any && !d_content) return CHIP_ERR_INVALID_ARG;
    const fread::ReadLayout lay(nreq, p.nseg, p.stage_total, p.vseg, nstreams);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    // the vouched read of the rows: its own checks of the streams and the scratch address, its plan
    vread::Plan vp;
    std::vector<uint64_t> vclen(nreq);
    const int vst = vread::plan_vread(reinterpret_cast<uintptr_t>(d_streams), in_off, in_len,
                                      reinterpret_cast<uintptr_t>(d_hash), padding, chunk_len, nstreams, req_stream,
                                      p.vstart.data(), p.vlen.data(), nreq, reinterpret_cast<uintptr_t>(scr + lay.rows),
                                      p.vcoff.data(), vclen.data(), true, flags,
                                      reinterpret_cast<uintptr_t>(scr + lay.vread), ~0ull, &vp);
    if (vst == CHIP_ERR_INVALID_ARG) return vst;
    if (rules::ranges_overlap(content_off, content_len, nreq)) return CHIP_ERR_INVALID_ARG;
    if (p.nseg >= (uint64_t(1) << 31) || scratch_len < lay.total) return CHIP_ERR_INVALID_ARG;
    if (vst != CHIP_OK) return vst;
    cread::Plan cp;
    if (format == 15) {
        st = cread::plan_ctr(keys, ivs, nstreams, req_stream, p.pos.data(), vclen.data(), nreq,
                             reinterpret_cast<uintptr_t>(scr + lay.rows), p.vcoff.data(),
                             reinterpret_cast<uintptr_t>(scr + lay.ctr), scratch_len - lay.ctr, nullptr, &cp);
    }
    const auto fail = [&](int code) {
        host::secure_wipe(cp.table.data(), cp.table.size());
        return code;
    };
    if (st != CHIP_OK) return fail(st);
    st = use_device();
    if (st != CHIP_OK) return fail(st);
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return fail(st);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    fread::plan_items(frame_off, idx_off, nframes, plain_len, index_status, req_stream, content_off, &p);
    if (h2d(c->stage, scr + lay.reqs, p.table.data(), p.table.size(), hs) != hipSuccess) return fail(CHIP_ERR_DEVICE);
    st = vread_enqueue(vp, d_status, d_used, d_vouch, flags, scr + lay.vread, stream);
    if (st != CHIP_OK) return fail(st);
    if (format == 15) {
        st = ctr_enqueue(cp, scr + lay.rows, d_status, nullptr, nullptr, nullptr, scr + lay.ctr, stream);
        if (st != CHIP_OK) return st;
    }
    FrameLaunch L{};
    L.reqs = reinterpret_cast<const fread::Req *>(scr + lay.reqs);
    L.segs = reinterpret_cast<const fread::Seg *>(scr + lay.segs);
    L.bad = reinterpret_cast<uint32_t *>(scr + lay.bad);
    L.rows = scr + lay.rows;
    L.content = d_content;
    L.status = d_status;
    L.used = d_used;
    L.vouch = d_vouch;
    L.nreq = uint32_t(nreq);
    L.nseg = uint32_t(p.nseg);
    CHIP_HIP(fread_block_launch(L, hs));
    CHIP_HIP(fread_finish_launch(L, hs));
    return CHIP_OK;
}

}  // extern "C"
