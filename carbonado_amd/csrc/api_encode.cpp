// api_encode.cpp — encode() from host memory (encoding.rs:86-172): one
// object (chip_encode) and the pipelined host batch (chip_encode_host_batch:
// host stages on host threads, H2D, K13, split copy-back).  Shared
// declarations: api_common.hpp.
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>

#include "api_common.hpp"

using namespace chip;
using namespace chip::api;

extern "C" {

// ---- pipeline glue -------------------------------------------------------

int chip_encode(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                uint8_t hash[CHIP_HASH_LEN], chip_encode_info *info) {
    if ((!in && n) || !out_len || !hash) return CHIP_ERR_INVALID_ARG;
    if ((format & CHIP_FORMAT_ECIES) && !pubkey) return CHIP_ERR_INVALID_ARG;
    // host stages (encoding.rs:101-115)
    thread_local std::vector<uint8_t> t_stage;
    thread_local Scratch t_tmp;
    const uint8_t *cur = in;
    uint64_t cur_n = n, bc = 0, be = 0;
    if (has_host_stages(format)) {
        Trace trace("host stages");
        // straight into the context's pinned input when a device stage follows
        // (the single-object paths then read it there, the others DMA it from
        // there): no copy of the staged bytes into pinned memory afterwards
        const uint64_t cap = host_stage_max(format, n) + 1;
        uint8_t *dst = nullptr;
        Ctx *c = nullptr;
        if ((format & (CHIP_FORMAT_ZFEC | CHIP_FORMAT_BAO)) && zc_ok(cap + 16) && ctx_get(&c) == CHIP_OK &&
            grow_pinned_local(c->hin, cap + 16) == hipSuccess)
            dst = static_cast<uint8_t *>(c->hin.p);
        if (!dst) {
            t_stage.resize(cap);
            dst = t_stage.data();
        }
        int st = host_stages_into(format, pubkey, pubkey_len, inject ? inject->ephemeral_sk : nullptr,
                                  inject ? inject->nonce : nullptr, in, n, dst, cap, t_tmp, &cur_n, &bc, &be, nullptr,
                                  nullptr, nullptr, true);
        if (st != CHIP_OK) return st;
        cur = dst;
        trace.mark("encode");
    }
    chip_encode_info inf;
    uint64_t cur_len, final_len;
    int st = encode_info_for(format, n, cur_n, bc, be, &inf, &cur_len, &final_len);
    if (st != CHIP_OK) return st;
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    if (final_len && (!out || out_cap < final_len)) return CHIP_ERR_BUFFER_TOO_SMALL;
    if (!zfec && !bao) {
        if (cur_n) std::memcpy(out, cur, cur_n);
        std::memset(hash, 0, 32);
    } else if (bao && single_ok(cur_len)) {  // one object on KM (split copy-back) or KS, zero-copy (api_single.cpp)
        Ctx *c;
        st = ctx_get(&c);
        if (st != CHIP_OK) return st;
        st = single_encode_km(c, cur, cur_n, zfec ? inf.chunk_len : 0, final_len, out, hash);
        if (st != CHIP_OK) return st;
    } else if (zfec && !bao && cur_n && zc_ok((uint64_t)CHIP_FEC_M * inf.chunk_len)) {  // encoding.rs:121-138 alone: zero-copy parity
        Ctx *c;
        st = ctx_get(&c);
        if (st != CHIP_OK) return st;
        st = single_zfec_encode_zc(c, cur, cur_n, inf.chunk_len, out);
        if (st != CHIP_OK) return st;
        std::memset(hash, 0, 32);  // encoding.rs:145
    } else {
        Ctx *c;
        st = ctx_get(&c);
        if (st != CHIP_OK) return st;
        CHIP_HIP(grow(c->in, cur_n));
        if (cur_n) CHIP_HIP(h2d(c->stage, c->in.p, cur, cur_n, c->stream));
        const uint8_t *d_cur = static_cast<const uint8_t *>(c->in.p);
        if (zfec && bao && cur_len) {  // fused: shards written into the bao stream, hashed in place
            CHIP_HIP(grow(c->out, final_len));
            CHIP_HIP(grow(c->scratch, std::max(zfec_bao_scratch_len(cur_len, 1), bao_scratch_len(cur_len, 1))));
            CHIP_HIP(grow(c->small, 64));
            uint8_t *d_hash = static_cast<uint8_t *>(c->small.p);
            CHIP_HIP(zfec_bao_dev(d_cur, 0, cur_n, 1, inf.chunk_len, static_cast<uint8_t *>(c->out.p), 0, d_hash,
                                  c->scratch.p, c->stream));
            CHIP_HIP(small_d2h(c, hash, d_hash, 32));
            CHIP_HIP(d2h(c->stage, out, c->out.p, final_len, c->stream));
            CHIP_HIP(small_sync(c));
            *out_len = final_len;
            if (info) *info = inf;
            return CHIP_OK;
        }
        if (zfec && cur_len) {
            CHIP_HIP(grow(c->mid, cur_len));
            GfPlan p = encode_plan(CHIP_FEC_K, CHIP_FEC_M, inf.chunk_len, zfec_enc_matrix(CHIP_FEC_K, CHIP_FEC_M));
            GfLaunch L{d_cur, static_cast<uint8_t *>(c->mid.p), 0, 0, cur_n, inf.chunk_len, 1};
            CHIP_HIP(gf_apply(p, L, c->stream));
            d_cur = static_cast<const uint8_t *>(c->mid.p);
        }
        if (bao) {  // encoding.rs:140-142: the zfec output stays on the device
            st = bao_encode_ctx(c, d_cur, cur_len, true, hash);
            if (st != CHIP_OK) return st;
            CHIP_HIP(d2h(c->stage, out, c->out.p, final_len, c->stream));
        } else {
            std::memset(hash, 0, 32);  // encoding.rs:145
            if (final_len) CHIP_HIP(d2h(c->stage, out, d_cur, final_len, c->stream));
        }
        CHIP_HIP(small_sync(c));
    }
    *out_len = final_len;
    if (info) *info = inf;
    return CHIP_OK;
}

namespace {

using hostbatch::HostGeo;

// encode() at Zfec|Bao from host memory, split copy-back: the stream's data
// region [0, t0) -- its header, the data-shard chunks [0, nh) and the parent
// nodes between them -- is half of the stream, and all of it but the nodes
// is the zero-padded input the host already holds (hostbatch::HostGeo at
// (1024 N, N / 2)).  The host writes the header and those chunks itself
// (host::fill_data_chunks, while it stages the slice); the device gathers the
// region's nodes into a compact buffer (bao_data_nodes); only that buffer and
// the tail [t0, final) cross PCIe, and the host scatters the nodes into their
// slots once the slot's stream is done.  D2H per 16 MiB object: 18.9 MB
// instead of 35.7.  CHIP_E2E_SPLIT=0: copy the whole stream back.
// CHIP_E2E_DIRECT=0: Ecies objects go through the pinned staging rows.
// CHIP_ECIES_PREP=0: each object's scalar multiplications inside its host stage.

// per-call cache of the split copy-back's geometry by chunk count (objects of a call may differ)
struct SplitGeos {
    std::mutex mu;
    std::map<uint64_t, HostGeo> by_n;
    const HostGeo &get(uint64_t N) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = by_n.find(N);
        if (it == by_n.end()) it = by_n.emplace(N, hostbatch::host_geo(1024 * N, N / 2, false)).first;
        return it->second;
    }
};

// The ECIES key material of a slice's objects (host::ecies_prepare: two
// scalar multiplications each, no data) computed on nt threads while the
// caller waits for the slice's slot: the slot wait is host time the data
// stages cannot use, the key material is the part of them that does not
// need the data.  The caller claims objects too once its wait is over.
struct KeyPrep {
    std::vector<host::EciesKey> keys;
    std::vector<int> sts;
    std::atomic<uint64_t> next{0};
    uint64_t cnt = 0;
    const uint8_t *peer = nullptr, *eph = nullptr;  // eph: injected secrets of the slice's objects
    std::vector<std::thread> pool;
    void claim() {
        for (uint64_t j; (j = next.fetch_add(1, std::memory_order_relaxed)) < cnt;)
            sts[j] = host::ecies_prepare(peer, eph ? eph + 32 * j : nullptr, &keys[j]);
    }
    void start(uint32_t nt, const uint8_t *peer_, const uint8_t *eph_, uint64_t cnt_) {
        if (keys.size() < cnt_) keys.resize(cnt_), sts.resize(cnt_);
        peer = peer_, eph = eph_, cnt = cnt_;
        next.store(0, std::memory_order_relaxed);
        for (uint32_t t = 0; t < nt; ++t) pool.emplace_back([this] { claim(); });
    }
    void finish() {
        claim();
        for (auto &th : pool) th.join();
        pool.clear();
    }
    void wipe() {
        for (uint64_t j = 0; j < cnt; ++j) host::ecies_key_wipe(&keys[j]);
    }
    ~KeyPrep() {
        for (auto &th : pool) th.join();
        wipe();
    }
};

// CHIP_E2E_TRACE=1: where a chip_encode_host_batch call's wall time went
// (host work of the slices on their threads, waits for a slot's stream, the final
// drain), one line on stderr per call
struct CallTrace {
    bool on = [] {
        const char *v = std::getenv("CHIP_E2E_TRACE");
        return v && v[0] == '1';
    }();
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double host = 0, host_max = 0, wait = 0, drain = 0, prep = 0;
    double now() const {
        return on ? std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() : 0.0;
    }
    void report(uint64_t slices, uint64_t S) const {
        if (!on) return;
        std::fprintf(stderr,
                     "[chip e2e] %llu slices of %llu: wall %.1f ms, host %.1f ms (slice max %.2f), "
                     "slot waits %.1f ms (with ECIES key prep %.1f ms), drain %.1f ms\n",
                     (unsigned long long)slices, (unsigned long long)S, now() * 1e3, host * 1e3, host_max * 1e3,
                     wait * 1e3, prep * 1e3, drain * 1e3);
    }
};

// a slice waiting for its nodes: cnt objects, compact buffers at hnodes + j * nstride
struct SplitPending {
    const HostGeo *g = nullptr;
    uint8_t *out = nullptr;
    uint64_t pitch = 0, cnt = 0, nstride = 0;
    const uint8_t *hnodes = nullptr;
    void scatter(uint64_t j) const {
        const uint8_t *src = hnodes + j * nstride;
        uint8_t *dst = out + j * pitch;
        for (const HostGeo::Run &r : g->runs) std::memcpy(dst + r.dst, src + r.src, r.len);
    }
};

// Device part of one slice of chip_encode_host_batch: cnt objects of cur_n
// bytes at src (host, pitch src_pitch) -> zfec -> bao -> out (host).  With
// split (Zfec|Bao only), the data region of every stream is the host's
// (HostGeo): the region's nodes go to sl.hnodes, the tail to out.
int batch_slice_device(Slot &sl, uint8_t format, const GfPlan *plan, const chip_encode_info &inf,
                       const uint8_t *src, uint64_t src_pitch, uint64_t cur_n, uint64_t zlen, uint64_t final_len,
                       uint64_t cnt, uint8_t *out, uint64_t out_pitch, uint8_t *hashes, uint64_t stream_off,
                       const HostGeo *split = nullptr, bool from_rows = false) {
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    // the streams 56 B into their rows: every chunk and node on a 64-B boundary
    // (K13, and K3 / the content mode for Bao alone; not KS, below 513 chunks)
    const bool any8 = bao && zlen &&
                      (zfec ? zfec_bao_any8(inf.chunk_len, cnt) : (zlen + 1023) / 1024 > KS_MAX_N);
    const uint64_t soff = any8 ? stream_off : 0;
    const uint64_t n_al = row_pitch(cur_n), z_al = row_pitch(zlen), f_al = row_pitch(final_len + soff);
    uint8_t *d_in = static_cast<uint8_t *>(sl.in.p);
    if (from_rows && split && cur_n) {
        // the host stage wrote each object's zfec input into its stream's chunk slots
        // in out: the data regions come over and the chunks are gathered into rows
        const uint64_t t_al = row_pitch(split->t0);
        uint8_t *d_sin = static_cast<uint8_t *>(sl.sin.p);
        CHIP_HIP(hipMemcpy2DAsync(d_sin, t_al, out, out_pitch, split->t0, cnt, hipMemcpyHostToDevice, sl.stream));
        CHIP_HIP(bao_gather_rows(d_sin, t_al, split->N, cnt, cur_n, d_in, n_al, sl.stream));
    } else if (cur_n) {
        CHIP_HIP(hipMemcpy2DAsync(d_in, n_al, src, src_pitch, cur_n, cnt, hipMemcpyHostToDevice, sl.stream));
    }
    const uint8_t *d_cur = d_in;
    uint64_t cur_stride = n_al;
    if (zfec && bao && zlen) {  // fused: shards written into the bao streams, hashed in place
        uint8_t *d_str = static_cast<uint8_t *>(sl.out.p) + soff;
        CHIP_HIP(zfec_bao_dev(d_in, n_al, cur_n, cnt, inf.chunk_len, d_str, f_al, static_cast<uint8_t *>(sl.hash.p),
                              sl.scratch.p, sl.stream));
        CHIP_HIP(hipMemcpyAsync(hashes, sl.hash.p, 32 * cnt, hipMemcpyDeviceToHost, sl.stream));
        if (split) {
            const uint64_t ns = split->nbytes;
            if (ns) {
                CHIP_HIP(bao_data_nodes(d_str, f_al, split->N, split->nh, cnt, static_cast<uint8_t *>(sl.nodes.p), ns,
                                        sl.stream));
                CHIP_HIP(hipMemcpyAsync(sl.hnodes.p, sl.nodes.p, cnt * ns, hipMemcpyDeviceToHost, sl.stream));
            }
            CHIP_HIP(hipMemcpy2DAsync(out + split->t0, out_pitch, d_str + split->t0, f_al, final_len - split->t0, cnt,
                                      hipMemcpyDeviceToHost, sl.stream));
        } else if (final_len) {
            CHIP_HIP(hipMemcpy2DAsync(out, out_pitch, d_str, f_al, final_len, cnt, hipMemcpyDeviceToHost, sl.stream));
        }
        return CHIP_OK;
    }
    if (zfec) {
        GfLaunch L{d_in, static_cast<uint8_t *>(sl.mid.p), n_al, z_al, cur_n, inf.chunk_len, cnt};
        CHIP_HIP(gf_apply(*plan, L, sl.stream));
        d_cur = static_cast<const uint8_t *>(sl.mid.p);
        cur_stride = z_al;
    }
    const uint8_t *d_res = d_cur;
    uint64_t res_stride = cur_stride;
    if (bao) {
        CHIP_HIP(bao_encode_dev(d_cur, cur_stride, zlen, cnt, static_cast<uint8_t *>(sl.out.p) + soff, f_al,
                                static_cast<uint8_t *>(sl.hash.p), sl.scratch.p, sl.stream));
        d_res = static_cast<const uint8_t *>(sl.out.p) + soff;
        res_stride = f_al;
        CHIP_HIP(hipMemcpyAsync(hashes, sl.hash.p, 32 * cnt, hipMemcpyDeviceToHost, sl.stream));
    } else {
        for (uint64_t o = 0; o < cnt; ++o) std::memset(hashes + 32 * o, 0, 32);
    }
    if (final_len)
        CHIP_HIP(hipMemcpy2DAsync(out, out_pitch, d_res, res_stride, final_len, cnt, hipMemcpyDeviceToHost,
                                  sl.stream));
    return CHIP_OK;
}

struct EncodeArgs {  // of chip_encode_host_batch, checked
    uint8_t format;
    const uint8_t *pubkey; uint64_t pubkey_len; const chip_ecies_inject *inject;
    const uint8_t *in; uint64_t n, count, in_stride;
    uint8_t *out; uint64_t out_stride, *out_len; uint8_t *hashes; chip_encode_info *info;
};

// One chip_encode_host_batch call with a device or host stage: plan,
// prepare_slots, then per slice wait_slot, host_slice, slice_infos and
// device_slice, then finish.
struct EncodeBatch : EncodeArgs {
    hostbatch::EncodeBounds b;
    const bool hs = has_host_stages(format), zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    Ctx *c = nullptr;  // null: host stages only
    hostbatch::Slices p{};
    uint64_t h_al = 0;  // pinned staging pitch
    // split copy-back (HostGeo): Zfec|Bao streams of at least 2 chunks; direct: with
    // ECIES, the host stage writes each stream's data region straight into out
    // (pinned), which the device then reads: no staging copy at all
    bool split_fmt = false, direct_fmt = false;
    // ECIES on the streaming path: the receiver key parsed once, each slice's
    // key material prepared during its slot wait (KeyPrep)
    bool prep = false;
    uint64_t soff_cfg = 0;  // where K13's streams sit in the slot rows (this call)
    SplitGeos geos;
    std::vector<uint8_t> enc;           // the zfec encode matrix
    std::vector<SplitPending> pend;     // per slot: the slice whose nodes are still to be placed
    std::vector<uint8_t> stage_host;    // host stages without a device part
    std::vector<Scratch> scratch;       // per host thread, reused across slices
    std::vector<uint64_t> len, bc, be;  // per object of the slice: the host stages' output lengths
    std::vector<uint64_t> zl, fl;       // ... and its zfec and final lengths
    std::vector<chip_encode_info> infs;
    std::vector<int> sts;
    std::vector<uint8_t> in_rows;  // object's data region written straight into out (direct)
    uint8_t peer[65];
    KeyPrep kp;
    CallTrace tr;
    // the slice in hand
    Slot *sl = nullptr;
    uint64_t o0 = 0, cnt = 0;
    const uint8_t *src = nullptr;  // what the device stages read: cnt objects of len[j] bytes
    uint64_t src_pitch = 0;
    bool uniform = true, rows = false;  // one length; all data regions already in out (direct)
    // the geometry an incompressible object's stream will have: ECIES places
    // its chunks block by block against it (host::ChunkSink)
    uint64_t n_pred = 0;
    const HostGeo *g_pred = nullptr;
    bool direct = false;

    const uint8_t *eph(uint64_t o) const {
        return inject && inject->ephemeral_sk ? inject->ephemeral_sk + 32 * o : nullptr;
    }
    const uint8_t *nonce(uint64_t o) const { return inject && inject->nonce ? inject->nonce + 16 * o : nullptr; }
    uint8_t *stage() { return sl ? static_cast<uint8_t *>(sl->stage.p) : stage_host.data(); }
    SplitPending &pending() { return pend[(o0 / p.S) % p.nslots]; }  // this slot's previous slice

    int plan(uint32_t nslots, uint64_t slice_bytes, uint32_t host_threads) {
        if (zfec || bao) {
            const int st = ctx_get(&c);
            if (st != CHIP_OK) return st;
        }
        // host work per object (host stages, split copy-back): slices in equal shares
        p = hostbatch::plan_slices(nslots, slice_bytes, host_threads, std::thread::hardware_concurrency(), b.h_max,
                                   count, hs || (zfec && bao));
        h_al = rules::up16(b.h_max);
        static const bool split_on = env_default_on("CHIP_E2E_SPLIT"), direct_on = env_default_on("CHIP_E2E_DIRECT"),
                          prep_on = env_default_on("CHIP_ECIES_PREP");
        split_fmt = zfec && bao && c && split_on && b.zlen_max >= 2048;
        direct_fmt = split_fmt && hs && stream_encrypt_on() && direct_on && out && host_pinned(out);
        prep = (format & CHIP_FORMAT_ECIES) && stream_encrypt_on() && prep_on;
        soff_cfg = stream_offset();
        n_pred = split_fmt && hs ? hostbatch::split_chunks(b.h_max) : 0;
        return CHIP_OK;
    }

    int prepare_slots() {
        const uint64_t S = p.S, zmax = b.zlen_max;
        if (c) {
            if (c->slots.size() < p.nslots) c->slots.resize(p.nslots);
            for (uint32_t k = 0; k < p.nslots; ++k) {
                Slot &s = c->slots[k];
                if (!s.stream) CHIP_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
                CHIP_HIP(grow(s.in, S * row_pitch(b.h_max)));
                if (zfec && !bao) CHIP_HIP(grow(s.mid, S * row_pitch(zmax)));  // Zfec|Bao: fused
                if (bao) {
                    CHIP_HIP(grow(s.out, S * row_pitch(b.final_max + soff_cfg)));
                    CHIP_HIP(grow(s.scratch, zfec ? std::max(zfec_bao_scratch_len(zmax, S), bao_scratch_len(zmax, S))
                                                  : bao_scratch_len(zmax, S)));
                }
                CHIP_HIP(grow(s.hash, S * 32));
                if (hs) CHIP_HIP(grow_pinned(s.stage, S * h_al));
                if (split_fmt) {  // the data region's nodes: fewer than the stream's N chunks
                    CHIP_HIP(grow(s.nodes, S * 64 * (zmax / 1024)));
                    CHIP_HIP(grow_pinned(s.hnodes, S * 64 * (zmax / 1024)));
                    if (direct_fmt) CHIP_HIP(grow(s.sin, S * row_pitch(geos.get(zmax / 1024).t0)));
                }
            }
        } else {
            stage_host.resize(S * h_al);
        }
        enc = zfec_enc_matrix(CHIP_FEC_K, CHIP_FEC_M);
        pend.resize(p.nslots);
        scratch.resize(p.T);
        for (auto *v : {&len, &bc, &be, &zl, &fl}) v->resize(S);
        infs.resize(S), sts.resize(S), in_rows.resize(S);
        g_pred = n_pred >= 2 ? &geos.get(n_pred) : nullptr;
        direct = direct_fmt && g_pred;
        tr = CallTrace{};  // the clock starts with the slices
        return prep ? host::ecies_peer(pubkey, pubkey_len, peer) : CHIP_OK;
    }

    // slice i in hand once its slot's previous slice is done; its ECIES key material meanwhile
    int wait_slot(uint64_t i) {
        sl = c ? &c->slots[i % p.nslots] : nullptr;
        o0 = i * p.S, cnt = std::min(p.S, count - o0);
        if (prep) kp.start(std::min<uint64_t>(p.T, cnt), peer, eph(o0), cnt);
        const double t_a = tr.now();
        const hipError_t e = sl && i >= p.nslots ? hipStreamSynchronize(sl->stream) : hipSuccess;
        tr.wait += tr.now() - t_a;
        if (prep) kp.finish();
        if (e != hipSuccess) {
            set_device_error(e);
            return CHIP_ERR_DEVICE;
        }
        if (prep) tr.prep += tr.now() - t_a;
        for (uint64_t j = 0; prep && j < cnt; ++j)
            if (kp.sts[j] != CHIP_OK) return kp.sts[j];
        return CHIP_OK;
    }

    // object j of the slice on a host thread: its host stages, then the header
    // and data chunks of its stream (split copy-back)
    void stage_object(uint64_t j, Scratch &tmp) {
        const uint64_t o = o0 + j;
        const uint8_t *obj = in + o * in_stride;
        uint64_t olen = n, filled = 0;
        uint8_t *row = out + o * out_stride;
        in_rows[j] = 0;
        if (hs) {
            uint8_t *staged = stage() + j * h_al;
            const host::ChunkSink sink{row, g_pred ? g_pred->coff.data() : nullptr, g_pred ? g_pred->nh : 0, direct,
                                       1024 * n_pred};
            sts[j] = host_stages_into(format, pubkey, pubkey_len, eph(o), nonce(o), obj, n, direct ? nullptr : staged,
                                      h_al, tmp, &len[j], &bc[j], &be[j], g_pred ? &sink : nullptr, &filled,
                                      prep ? &kp.keys[j] : nullptr);
            if (sts[j] != CHIP_OK) return;
            olen = len[j];
            if (direct) {
                if (hostbatch::split_chunks(olen) == n_pred) {  // the data region is complete in out
                    host::fill_chunk_range(row, g_pred->coff.data(), filled, g_pred->nh, nullptr, 0);
                    in_rows[j] = 1;
                    return;
                }
                // another geometry (compressible input): the output back from the slots
                host::gather_chunks(staged, row, g_pred->coff.data(), olen);
                filled = 0;
            }
            obj = staged;
        }
        // the stream's header and data chunks (a ragged slice copies its
        // streams back whole over this; chunks placed against a wrong
        // prediction lie inside the stream and are overwritten too)
        const uint64_t N = split_fmt ? hostbatch::split_chunks(olen) : 0;
        if (N < 2) return;
        const HostGeo &g = geos.get(N);
        if (filled > 1 && N == n_pred) {  // chunks [1, filled) are in place
            host::fill_data_chunks(row, g.coff.data(), 1, 1024 * N, obj, olen);
            host::fill_chunk_range(row, g.coff.data(), filled, g.nh, obj, olen);
        } else {
            host::fill_data_chunks(row, g.coff.data(), g.nh, 1024 * N, obj, olen);
        }
    }

    // On T threads while earlier slices run on the device: the nodes of this
    // slot's previous slice into place, then this slice's host stages and the
    // data region of its streams.  Leaves src / src_pitch / len[] / uniform / rows.
    int host_slice() {
        src = in + o0 * in_stride;
        src_pitch = count > 1 ? in_stride : n;
        uniform = true, rows = false;
        for (uint64_t j = 0; j < cnt; ++j) len[j] = n, bc[j] = be[j] = 0;
        if (!hs && !split_fmt) return CHIP_OK;
        SplitPending &pp = pending();  // (its stream is done)
        const uint32_t nt = (uint32_t)std::min<uint64_t>(p.T, std::max(cnt, pp.g ? pp.cnt : 0));
        const double t_h = tr.now();
        run_threads(nt, [&](uint32_t t) {
            if (pp.g)
                for (uint64_t j = t; j < pp.cnt; j += nt) pp.scatter(j);
            for (uint64_t j = t; j < cnt; j += nt) stage_object(j, scratch[t]);
        });
        const double dh = tr.now() - t_h;
        tr.host += dh;
        tr.host_max = std::max(tr.host_max, dh);
        pp = SplitPending{};
        if (prep) kp.wipe();
        if (!hs) return CHIP_OK;
        for (uint64_t j = 0; j < cnt; ++j)
            if (sts[j] != CHIP_OK) return sts[j];
        src = stage();
        src_pitch = h_al;
        rows = direct;
        for (uint64_t j = 0; j < cnt; ++j) uniform &= len[j] == len[0], rows &= in_rows[j] != 0;
        rows &= uniform;
        if (direct && !rows)  // a ragged slice: from the staging rows, as without `direct`
            for (uint64_t j = 0; j < cnt; ++j)
                if (in_rows[j])
                    host::gather_chunks(stage() + j * h_al, out + (o0 + j) * out_stride, g_pred->coff.data(), len[j]);
        return CHIP_OK;
    }

    // per-object EncodeInfo (identical for a uniform slice); zl / fl kept for the dispatch
    int slice_infos() {
        for (uint64_t j = 0; j < cnt; ++j) {
            const int st = encode_info_for(format, n, len[j], bc[j], be[j], &infs[j], &zl[j], &fl[j]);
            if (st != CHIP_OK) return st;
            out_len[o0 + j] = fl[j];
            if (info) info[o0 + j] = infs[j];
        }
        return CHIP_OK;
    }

    // the slice's device stages enqueued on its slot's stream: one batched pass
    // over a uniform slice, one object at a time over a ragged one
    // (compressible data through the host stages)
    int device_slice() {
        if (!sl) {  // host stages only (no Zfec/Bao bit)
            for (uint64_t j = 0; j < cnt; ++j) {
                std::memcpy(out + (o0 + j) * out_stride, src + j * src_pitch, len[j]);
                std::memset(hashes + 32 * (o0 + j), 0, 32);
            }
            return CHIP_OK;
        }
        const uint64_t groups = uniform ? 1 : cnt, gcnt = uniform ? cnt : 1;
        for (uint64_t j = 0; j < groups; ++j) {
            const GfPlan gp = encode_plan(CHIP_FEC_K, CHIP_FEC_M, infs[j].chunk_len, enc);
            const HostGeo *g = uniform && split_fmt && zl[j] >= 2048 ? &geos.get(zl[j] / 1024) : nullptr;
            uint8_t *dst = out + (o0 + j) * out_stride;
            const uint64_t opitch = uniform && count > 1 ? out_stride : fl[j];
            const int st = batch_slice_device(*sl, format, &gp, infs[j], src + j * src_pitch, src_pitch, len[j], zl[j],
                                              fl[j], gcnt, dst, opitch, hashes + 32 * (o0 + j), soff_cfg, g,
                                              uniform && rows);
            if (st != CHIP_OK) return st;
            if (g) pending() = SplitPending{g, dst, opitch, cnt, g->nbytes, static_cast<const uint8_t *>(sl->hnodes.p)};
        }
        return CHIP_OK;
    }

    // the drain (the one error path's too), the trace report, the nodes of the last slices into place
    int finish(int st) {
        const double t_d = tr.now();
        hipError_t e = hipSuccess;
        for (uint32_t k = 0; c && k < p.nslots; ++k) {
            const hipError_t ek = hipStreamSynchronize(c->slots[k].stream);
            if (e == hipSuccess) e = ek;
        }
        if (st != CHIP_OK) return st;
        CHIP_HIP(e);
        tr.drain = tr.now() - t_d;
        tr.report(p.nslices, p.S);
        for (const SplitPending &pp : pend) {
            if (!pp.g) continue;
            const uint32_t nt = (uint32_t)std::min<uint64_t>(p.T, pp.cnt);
            run_threads(nt, [&pp, nt](uint32_t t) {
                for (uint64_t j = t; j < pp.cnt; j += nt) pp.scatter(j);
            });
        }
        return CHIP_OK;
    }
};

}  // namespace

int chip_encode_host_batch(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len,
                           const chip_ecies_inject *inject, const uint8_t *in, uint64_t n, uint64_t count,
                           uint64_t in_stride, uint8_t *out, uint64_t out_stride, uint64_t *out_len,
                           uint8_t *hashes, chip_encode_info *info, uint32_t nslots, uint64_t slice_bytes,
                           uint32_t host_threads) {
    if ((!in && n && count) || (!out_len && count) || (!hashes && count)) return CHIP_ERR_INVALID_ARG;
    if ((format & CHIP_FORMAT_ECIES) && !pubkey) return CHIP_ERR_INVALID_ARG;
    if (count > 1 && in_stride < n) return CHIP_ERR_INVALID_ARG;
    if (count == 0) return CHIP_OK;
    // sizes: exact without host stages, bounds with them
    const hostbatch::EncodeBounds b = hostbatch::encode_bounds(format, n);
    if (b.st != CHIP_OK) return b.st;
    if (count > 1 && out_stride < b.final_max) return CHIP_ERR_BUFFER_TOO_SMALL;
    if (b.final_max && !out) return CHIP_ERR_BUFFER_TOO_SMALL;
    if (!(format & (CHIP_FORMAT_ECIES | CHIP_FORMAT_SNAPPY | CHIP_FORMAT_ZFEC | CHIP_FORMAT_BAO))) {
        // format 0: identity, nothing for the device to do
        for (uint64_t o = 0; o < count; ++o) {
            if (n) std::memcpy(out + o * out_stride, in + o * in_stride, n);
            std::memset(hashes + 32 * o, 0, 32);
            out_len[o] = n;
            if (info) info[o] = b.inf;
        }
        return CHIP_OK;
    }
    EncodeBatch eb{{format, pubkey, pubkey_len, inject, in, n, count, in_stride, out, out_stride, out_len, hashes, info},
                   b};
    int st = eb.plan(nslots, slice_bytes, host_threads);
    if (st != CHIP_OK) return st;
    st = eb.prepare_slots();
    if (st != CHIP_OK) return st;
    for (uint64_t i = 0; i < eb.p.nslices && st == CHIP_OK; ++i) {
        st = eb.wait_slot(i);
        if (st == CHIP_OK) st = eb.host_slice();
        if (st == CHIP_OK) st = eb.slice_infos();
        if (st == CHIP_OK) st = eb.device_slice();
    }
    return eb.finish(st);
}

}  // extern "C"
