// api_decode.cpp — decode() from host memory (decoding.rs:80-114): one
// object (chip_decode) and the pipelined host batch (chip_decode_host_batch:
// H2D, bao verify-decode, D2H, host stages on host threads).  Shared
// declarations: api_common.hpp; the geometry: hostbatch_plan.hpp.
#include <condition_variable>
#include <mutex>
#include <thread>

#include "api_common.hpp"

using namespace chip;
using namespace chip::api;

namespace {

using hostbatch::DecGeom;

// decode()'s host stages (decoding.rs:101-111) on the device stages' output
// cur[0, cur_n) of ONE object: ECIES then snappy, or the two in one pass.
// The pooled implementations with the key derived ahead (when there is one):
// the caller's only object may take every thread of the stage pool, and its
// key was derived while the device verified.
int host_tail(const uint8_t *secret_key, uint64_t sk_len, bool ecies, bool snap, const uint8_t *cur, uint64_t cur_n,
              uint8_t *out, uint64_t out_cap, uint64_t *out_len, const uint8_t *pre_key, const uint8_t *pre_eph) {
    Trace trace("host stages");
    struct Mark {
        Trace &t;
        ~Mark() { t.mark("decode"); }
    } mark{trace};
    if (ecies && snap)  // decoding.rs:101-111 in one pass
        return host::ecies_decrypt_snap_par(secret_key, sk_len, cur, cur_n, out, out_cap, out_len, pre_key, pre_eph);
    if (ecies) {  // decoding.rs:101-105
        uint64_t got = 0;
        const int st = host::ecies_decrypt_par(secret_key, sk_len, cur, cur_n, out, out_cap, &got, pre_key, pre_eph);
        if (st == CHIP_OK || st == CHIP_ERR_BUFFER_TOO_SMALL) *out_len = got;
        return st;
    }
    return host::snap_decompress_par(cur, cur_n, out, out_cap, out_len);  // decoding.rs:107-111
}

// CHIP_DEC_SPEC=0: a decode's host stages wait for the device's verdict
// instead of running on the unverified content meanwhile (an A/B knob)
bool dec_spec_on() {
    static const bool on = [] {
        const char *e = std::getenv("CHIP_DEC_SPEC");
        return !(e && e[0] == '0');
    }();
    return on;
}

// Between the thread that enqueues a decode batch's slices and the finisher
// that completes them in order: how many slices each has done, and whether
// either gave up.
struct Handshake {
    std::mutex m;
    std::condition_variable cv;
    uint64_t enqueued = 0, finished = 0;
    bool aborted = false;
    // until slice i is enqueued; false: it never will be
    bool wait_enqueued(uint64_t i) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return enqueued > i || aborted; });
        return enqueued > i;
    }
    // until slice i is finished; false: the run is aborted
    bool wait_finished(uint64_t i) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return finished > i || aborted; });
        return !aborted;
    }
    // slice i through `step` (enqueued or finished), or with !ok the end of the run; false: the run is aborted
    bool publish(uint64_t &step, uint64_t i, bool ok) {
        std::lock_guard<std::mutex> lk(m);
        if (ok) step = i + 1;
        else aborted = true;
        cv.notify_all();
        return !aborted;
    }
};

struct DecodeArgs {  // of chip_decode_host_batch, checked
    uint8_t format;
    const uint8_t *secret_key; uint64_t sk_len;
    const uint8_t *hashes, *in; const uint64_t *in_len; uint64_t count, in_stride; const uint32_t *padding;
    uint8_t *out; uint64_t out_stride, *out_len; int32_t *status;
};

// One chip_decode_host_batch call: geometry, then either host_only, or plan,
// prepare_slots and run (enqueue on this thread, finish on the finisher's).
struct DecodeBatch : DecodeArgs {
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO, hs = has_host_stages(format);
    const bool ecies = format & CHIP_FORMAT_ECIES, snap = format & CHIP_FORMAT_SNAPPY;
    std::vector<DecGeom> geo;
    uint64_t in_max = 0, mid_max = 0, olen_max = 0;
    Ctx *c = nullptr;
    hostbatch::Slices p{};
    uint64_t i_al = 0, m_al = 0, o_al = 0;  // pitches: slot input rows, bao's output rows, the pinned stage's rows
    std::vector<Scratch> dscratch;          // per host thread, reused across slices
    Handshake hsk;
    std::string fin_err;

    // host-side geometry and the largest sizes
    void geometry() {
        geo.resize(count);
        for (uint64_t o = 0; o < count; ++o) {
            geo[o] = hostbatch::dec_geom(format, in + o * in_stride, in_len[o], padding[o]);
            status[o] = geo[o].st;
            in_max = std::max(in_max, in_len[o]);
            mid_max = std::max(mid_max, geo[o].blen);
            olen_max = std::max(olen_max, geo[o].olen);
        }
    }

    int first_error() const {
        for (uint64_t o = 0; o < count; ++o)
            if (status[o] != CHIP_OK) return status[o];
        return CHIP_OK;
    }

    // No Zfec/Bao bit: host stages only (or identity), the objects one after the
    // other on this thread.  The pooled implementations without a key derived
    // ahead: each object in its turn may take the stage pool, and there is no
    // device stage during which its key could have been derived.
    int host_only() {
        for (uint64_t o = 0; o < count; ++o) {
            if (status[o] != CHIP_OK) continue;
            const uint8_t *src = in + o * in_stride;
            const uint64_t n = in_len[o];
            uint8_t *dst = out + o * out_stride;
            uint64_t got = n;
            if (!hs) {
                if (n > out_stride && count > 1) status[o] = CHIP_ERR_BUFFER_TOO_SMALL;
                else std::memcpy(dst, src, n);
            } else {
                got = 0;
                if (ecies && snap)
                    status[o] = host::ecies_decrypt_snap_par(secret_key, sk_len, src, n, dst, out_stride, &got);
                else if (ecies) status[o] = host::ecies_decrypt_par(secret_key, sk_len, src, n, dst, out_stride, &got);
                else status[o] = host::snap_decompress(src, n, dst, out_stride, &got);
            }
            out_len[o] = got;
        }
        return first_error();
    }

    int plan(uint32_t nslots, uint64_t slice_bytes, uint32_t host_threads) {
        const int st = ctx_get(&c);
        if (st != CHIP_OK) return st;
        p = hostbatch::plan_slices(nslots, slice_bytes, host_threads, std::thread::hardware_concurrency(), in_max, count,
                                   false);
        i_al = row_pitch(in_max), m_al = row_pitch(mid_max), o_al = rules::up16(olen_max);
        dscratch.resize(p.T);
        return CHIP_OK;
    }

    int prepare_slots() {
        const uint64_t S = p.S;
        if (c->slots.size() < p.nslots) c->slots.resize(p.nslots);
        for (uint32_t k = 0; k < p.nslots; ++k) {
            Slot &sl = c->slots[k];
            if (!sl.stream) CHIP_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
            CHIP_HIP(grow(sl.in, S * i_al));
            if (bao) {
                CHIP_HIP(grow(sl.mid, S * m_al));
                CHIP_HIP(grow(sl.scratch, bao_scratch_len(mid_max, S)));
                CHIP_HIP(grow(sl.hash, S * 32 + S * 4));  // hashes, then per-object status words
            }
            if (hs) CHIP_HIP(grow_pinned(sl.stage, S * o_al + S * 4));
            else if (bao) CHIP_HIP(grow_pinned(sl.stage, S * 4));
        }
        return CHIP_OK;
    }

    // the status words of a slot's slice in its pinned stage (behind the rows of the host stages' input)
    uint32_t *stage_status(Slot &sl) const {
        return reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(sl.stage.p) + (hs ? p.S * o_al : 0));
    }

    // device part of slice i (H2D, bao verify, D2H) enqueued on its slot's stream
    int enqueue(uint64_t i) {
        Slot &sl = c->slots[i % p.nslots];
        const uint64_t S = p.S, o0 = i * S, cnt = std::min(S, count - o0);
        uint8_t *stage = static_cast<uint8_t *>(sl.stage.p);
        uint32_t *h_st = stage_status(sl);
        for (uint64_t j = 0; j < cnt; ++j) { h_st[j] = 0; if (!hs) out_len[o0 + j] = geo[o0 + j].olen; }
        // uniform slice -> one batched pass; otherwise object by object
        bool uniform = true;
        for (uint64_t j = 1; j < cnt; ++j)
            uniform &= in_len[o0 + j] == in_len[o0] && geo[o0 + j].blen == geo[o0].blen &&
                       geo[o0 + j].olen == geo[o0].olen;
        for (uint64_t j = 0; j < cnt; ++j) uniform &= geo[o0 + j].st == CHIP_OK;
        const uint64_t groups = uniform ? 1 : cnt;
        for (uint64_t gI = 0; gI < groups; ++gI) {
            const uint64_t j0 = uniform ? 0 : gI, gcnt = uniform ? cnt : 1, o = o0 + j0;
            if (geo[o].st != CHIP_OK) continue;
            const uint64_t n = in_len[o], blen = geo[o].blen, olen = geo[o].olen;
            uint8_t *d_in = static_cast<uint8_t *>(sl.in.p) + j0 * i_al;
            if (n) CHIP_HIP(hipMemcpy2DAsync(d_in, i_al, in + o * in_stride, count > 1 ? in_stride : n, n, gcnt,
                                             hipMemcpyHostToDevice, sl.stream));
            const uint8_t *d_res = d_in;
            uint64_t res_pitch = i_al;
            if (bao) {  // decoding.rs:89-93, all objects of the group verified in one pass
                uint8_t *d_hash = static_cast<uint8_t *>(sl.hash.p) + j0 * 32;
                uint32_t *d_st = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(sl.hash.p) + S * 32) + j0;
                CHIP_HIP(hipMemcpyAsync(d_hash, hashes + 32 * o, 32 * gcnt, hipMemcpyHostToDevice, sl.stream));
                CHIP_HIP(hipMemsetAsync(d_st, 0, 4 * gcnt, sl.stream));
                uint8_t *d_mid = static_cast<uint8_t *>(sl.mid.p) + j0 * m_al;
                // every byte verified; only the bytes zfec keeps (the data shards) written
                // (CHIP_DECODE_PREFIX=0: round 4's whole-content verify-decode, the A/B of DESIGN §6)
                static const bool prefix = env_int("CHIP_DECODE_PREFIX", 1) != 0;
                if (prefix)
                    CHIP_HIP(bao_decode_prefix_dev(d_in, i_al, blen, gcnt, d_hash, d_mid, m_al, zfec ? olen : blen,
                                                   d_st, sl.scratch.p, sl.stream));
                else
                    CHIP_HIP(bao_decode_dev(d_in, i_al, blen, gcnt, d_hash, d_mid, m_al, d_st, sl.scratch.p,
                                            sl.stream));
                CHIP_HIP(hipMemcpyAsync(h_st + j0, d_st, 4 * gcnt, hipMemcpyDeviceToHost, sl.stream));
                d_res = d_mid;
                res_pitch = m_al;
            }
            // zfec (decoding.rs:95-99): the shards are indexed by position, so the
            // primaries are present and decode = their bytes, padding dropped
            if (olen) {
                uint8_t *dst = hs ? stage + j0 * o_al : out + o * out_stride;
                const uint64_t dpitch = hs ? o_al : (count > 1 ? out_stride : olen);
                if (!hs && count > 1 && olen > out_stride) {
                    for (uint64_t j = 0; j < gcnt; ++j) status[o + j] = CHIP_ERR_BUFFER_TOO_SMALL;
                    continue;
                }
                CHIP_HIP(hipMemcpy2DAsync(dst, dpitch, d_res, res_pitch, olen, gcnt, hipMemcpyDeviceToHost, sl.stream));
            }
        }
        return CHIP_OK;
    }

    // Host part of slice i, its slot's stream done: device statuses -> status[],
    // then ecies -> snap into out, an object per thread on T threads.  The
    // one-thread implementations with the thread's own scratch: the threads are
    // already busy with an object each, so the stage pool would only be fought over.
    void finish(uint64_t i) {
        Slot &sl = c->slots[i % p.nslots];
        const uint64_t o0 = i * p.S, cnt = std::min(p.S, count - o0);
        const uint8_t *stage = static_cast<const uint8_t *>(sl.stage.p);
        const uint32_t *dst_st = stage_status(sl);
        for (uint64_t j = 0; j < cnt; ++j)
            if (bao && status[o0 + j] == CHIP_OK && dst_st[j]) status[o0 + j] = (int32_t)dst_st[j];
        if (!hs) return;
        const uint32_t nt = (uint32_t)std::min<uint64_t>(p.T, cnt);
        run_threads(nt, [&](uint32_t t) {
            for (uint64_t j = t; j < cnt; j += nt) {
                const uint64_t o = o0 + j, n = geo[o].olen;
                if (status[o] != CHIP_OK) continue;
                const uint8_t *src = stage + j * o_al;
                uint8_t *dst = out + o * out_stride;
                uint64_t got = 0;
                if (ecies && snap)  // one pass, no plaintext buffer
                    status[o] = host::ecies_decrypt_snap(secret_key, sk_len, src, n, dst, out_stride, &got,
                                                         dscratch[t].get(host::DECRYPT_SNAP_WINDOW));
                else if (ecies) status[o] = host::ecies_decrypt(secret_key, sk_len, src, n, dst, out_stride, &got);
                else status[o] = host::snap_decompress(src, n, dst, out_stride, &got);
                out_len[o] = got;
            }
        });
    }

    // the finisher's thread: slices in order, each once its slot's stream is done
    void finisher_loop() {
        (void)hipSetDevice(c->dev);
        for (uint64_t i = 0; i < p.nslices && hsk.wait_enqueued(i); ++i) {
            const hipError_t e = hipStreamSynchronize(c->slots[i % p.nslots].stream);
            if (e == hipSuccess) finish(i);
            else fin_err = hipGetErrorString(e);
            if (!hsk.publish(hsk.finished, i, e == hipSuccess)) return;
        }
    }

    // A finisher thread completes slices in order (wait for the slot's stream,
    // then the host stages on T threads) while this thread keeps the device
    // queue full; a slot is reused only after its previous slice finished.
    int run() {
        std::thread finisher([this] { finisher_loop(); });
        int st = CHIP_OK;
        for (uint64_t i = 0; i < p.nslices && st == CHIP_OK; ++i) {
            if (i >= p.nslots && !hsk.wait_finished(i - p.nslots)) {
                st = CHIP_ERR_DEVICE;
                break;
            }
            st = enqueue(i);
            hsk.publish(hsk.enqueued, i, st == CHIP_OK);
        }
        finisher.join();
        if (!fin_err.empty()) {
            t_last_err = fin_err;
            st = CHIP_ERR_DEVICE;
        }
        hipError_t e = hipSuccess;
        for (uint32_t k = 0; k < p.nslots; ++k) {
            const hipError_t ek = hipStreamSynchronize(c->slots[k].stream);
            if (e == hipSuccess) e = ek;
        }
        if (st != CHIP_OK) return st;
        CHIP_HIP(e);
        return first_error();
    }
};

}  // namespace

extern "C" {

int chip_decode_host_batch(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *hashes,
                           const uint8_t *in, const uint64_t *in_len, uint64_t count, uint64_t in_stride,
                           const uint32_t *padding, uint8_t *out, uint64_t out_stride, uint64_t *out_len,
                           int32_t *status, uint32_t nslots, uint64_t slice_bytes, uint32_t host_threads) {
    if (count == 0) return CHIP_OK;
    if (!in || !in_len || !out_len || !status || !padding) return CHIP_ERR_INVALID_ARG;
    if ((format & CHIP_FORMAT_ECIES) && !secret_key) return CHIP_ERR_INVALID_ARG;
    if ((format & CHIP_FORMAT_BAO) && !hashes) return CHIP_ERR_HASH_DECODE;
    DecodeBatch db{{format, secret_key, sk_len, hashes, in, in_len, count, in_stride, padding, out, out_stride, out_len,
                    status}};
    db.geometry();
    if (!db.zfec && !db.bao) return db.host_only();
    int st = db.plan(nslots, slice_bytes, host_threads);
    if (st == CHIP_OK) st = db.prepare_slots();
    return st == CHIP_OK ? db.run() : st;
}

int chip_decode(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *hash, uint64_t hash_len,
                const uint8_t *in, uint64_t n, uint32_t padding, uint8_t format, uint8_t *out, uint64_t out_cap,
                uint64_t *out_len) {
    if ((!in && n) || !out_len) return CHIP_ERR_INVALID_ARG;
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    const bool ecies = format & CHIP_FORMAT_ECIES, snap = format & CHIP_FORMAT_SNAPPY;
    if (ecies && !secret_key) return CHIP_ERR_INVALID_ARG;
    // device stages write to `out` directly unless host stages follow
    thread_local std::vector<uint8_t> t_dev;
    const uint8_t *cur = in;
    uint64_t cur_n = n;
    uint8_t pre_eph[65], pre_key[32];  // ECIES key derived while the device works
    bool have_pre = false;
    struct Wipe {
        uint8_t *k;
        ~Wipe() { host::secure_wipe(k, 32); }
    } wipe_pre{pre_key};
    if (zfec || bao) {
        if (bao && (!hash || hash_len != CHIP_HASH_LEN)) return CHIP_ERR_HASH_DECODE;
        const DecGeom g = hostbatch::dec_geom(format, in, n, padding);
        if (g.st != CHIP_OK) return g.st;
        const uint64_t blen = g.blen, olen = g.olen, C = zfec ? blen / CHIP_FEC_M : 0;
        if (C % 16) return CHIP_ERR_ZFEC;
        uint8_t *dst = out;
        if (ecies || snap) {
            t_dev.resize(olen + 1);
            dst = t_dev.data();
        } else if (olen && (!out || out_cap < olen)) {
            *out_len = olen;
            return CHIP_ERR_BUFFER_TOO_SMALL;
        }
        Ctx *c;
        int st = ctx_get(&c);
        if (st != CHIP_OK) return st;
        // While the device works: the ECIES key from the envelope header as the
        // input holds it at h0 (content bytes [0, 65): chunk 0 of the bao stream, or
        // the first shard); decrypt uses it only if the verified header is the same
        // (the pool path and the one-thread paths alike, so it is never paid twice)
        const uint64_t h0 = ecies && bao ? bao_chunk_offset(0, (blen + 1023) / 1024) : 0;
        auto prekey = [&](uint64_t at) {
            if (!ecies || at + 65 > n || (bao && blen < 65)) return;
            std::memcpy(pre_eph, in + at, 65);
            have_pre = host::ecies_derive_key(secret_key, sk_len, pre_eph, pre_key) == CHIP_OK;
        };
        if (bao && single_ok(blen)) {  // KM / KS verifies; the host gathers [0, olen) from `in` meanwhile
            // (at Bao|Zfec the positional shares' primaries are the content's first 4 C bytes)
            // and then the host stages themselves on the gathered (still unverified) content,
            // into `out`: released only with the device's verdict, wiped without it
            int spec = -1;
            const uint64_t out_len0 = *out_len;
            auto stages = [&] {
                if (!(ecies || snap) || !dec_spec_on() || (ecies && !have_pre)) return;
                spec = host_tail(secret_key, sk_len, ecies, snap, dst, olen, out, out_cap, out_len, pre_key, pre_eph);
            };
            st = single_decode_km(c, in, n, blen, hash, dst, olen, [&] { prekey(h0); }, stages);
            if (spec >= 0) {
                if (st == CHIP_OK) return spec;
                if (out && out_cap) host::secure_wipe(out, spec == CHIP_OK ? *out_len : out_cap);
                *out_len = out_len0;
            }
            if (st != CHIP_OK) return st;
        } else if (zfec && !bao && C && zc_ok(2 * CHIP_FEC_K * C)) {  // decoding.rs:95-99: shards by position
            // zero-copy: the decode kernel reads the four primaries from pinned memory
            const uint8_t *sh[CHIP_FEC_K];
            std::vector<uint32_t> sel(CHIP_FEC_K);
            for (uint32_t s = 0; s < CHIP_FEC_K; ++s) { sh[s] = in + s * C; sel[s] = s; }
            st = single_zfec_decode_zc(c, CHIP_FEC_K, CHIP_FEC_M, sh, sel, C, dst, olen, [&] { prekey(0); });
            if (st != CHIP_OK) return st;
        } else {
            const uint64_t in_bytes = bao ? bao_encoded_len(blen) : n;
            CHIP_HIP(grow(c->in, in_bytes));
            if (in_bytes) CHIP_HIP(h2d(c->stage, c->in.p, in, in_bytes, c->stream));
            const uint8_t *d_cur = static_cast<const uint8_t *>(c->in.p);
            uint32_t verdict = 0;  // bao's, read at the synchronisation below
            if (bao && zfec) {  // decoding.rs:89-99: the positional shares' primaries are the content's
                // first 4 C bytes, so zfec's decode is the prefix: verify all, write olen bytes
                CHIP_HIP(grow(c->mid, olen));
                st = bao_decode_ctx(c, d_cur, in_bytes, blen, hash, static_cast<uint8_t *>(c->mid.p), olen, &verdict);
                if (st != CHIP_OK) return st;
                d_cur = static_cast<const uint8_t *>(c->mid.p);
            } else if (bao) {  // decoding.rs:89-93
                CHIP_HIP(grow(c->mid, blen));
                st = bao_decode_ctx(c, d_cur, in_bytes, blen, hash, static_cast<uint8_t *>(c->mid.p), ~0ull, &verdict);
                if (st != CHIP_OK) return st;
                d_cur = static_cast<const uint8_t *>(c->mid.p);
            }
            if (zfec && !bao && C) {  // decoding.rs:95-99: shards by position, primaries present
                CHIP_HIP(grow(c->out, CHIP_FEC_K * C));
                std::vector<uint32_t> sel(CHIP_FEC_K);
                std::vector<uint64_t> slot_off(CHIP_FEC_K);
                for (uint32_t s = 0; s < CHIP_FEC_K; ++s) { sel[s] = s; slot_off[s] = s * C; }
                st = zfec_decode_device(CHIP_FEC_K, CHIP_FEC_M, d_cur, 0, slot_off, sel, C, 1,
                                        static_cast<uint8_t *>(c->out.p), 0, c->stream);
                if (st != CHIP_OK) return st;
                d_cur = static_cast<const uint8_t *>(c->out.p);
            }
            prekey(h0);
            if (olen) CHIP_HIP(d2h(c->stage, dst, d_cur, olen, c->stream));
            CHIP_HIP(small_sync(c));
            if (verdict) {  // never hand back unverified content
                if (olen) std::memset(dst, 0, olen);
                return (int)verdict;
            }
        }
        cur = dst;
        cur_n = olen;
    }
    if (!ecies && !snap) {
        if (!(zfec || bao)) {
            if (n && (!out || out_cap < n)) {
                *out_len = n;
                return CHIP_ERR_BUFFER_TOO_SMALL;
            }
            if (n) std::memcpy(out, in, n);
        }
        *out_len = cur_n;
        return CHIP_OK;
    }
    return host_tail(secret_key, sk_len, ecies, snap, cur, cur_n, out, out_cap, out_len, have_pre ? pre_key : nullptr,
                     pre_eph);
}

}  // extern "C"
