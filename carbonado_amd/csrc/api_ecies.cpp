// api_ecies.cpp — the AES-256-GCM calls of include/carbonado_hip_ecies.h over
// device-resident messages.  The checks, the scratch layout and the table are
// host code in ecies_plan.hpp; this file uploads the table (through a pinned
// copy that a host function wipes behind the upload), enqueues the kernels of
// ecies_kernels.hip and, last, the memset that zeroes the key region.  The
// envelope and one-call forms take the place the AES keys come from as a
// parameter (api_agree.hpp): the stage pool's threads for the chipe_* calls,
// the key agreement kernels for the chipy_* calls of api_agree.cpp.
#include "api_agree.hpp"
#include "api_common.hpp"
#include "ecies_kernels.hpp"
#include "ecies_plan.hpp"
#include "key_upload.hpp"
#include "ragged_plan.hpp"

#include <openssl/rand.h>

using namespace chip;
using namespace chip::api;

namespace {

GcmLaunch launch_of(const ecies::Plan &p, uint8_t *scr, const uint8_t *d_in, uint8_t *d_out, uint8_t *d_tag,
                    uint32_t *d_status) {
    GcmLaunch L{};
    L.msgs = reinterpret_cast<const gcm::Msg *>(scr + p.lay.msgs);
    L.rawkeys = scr + p.lay.keys;
    L.km = reinterpret_cast<gcm::KeyMat *>(scr + p.lay.km);
    L.vals = reinterpret_cast<gcm::B128 *>(scr + p.lay.vals);
    L.ok = reinterpret_cast<uint32_t *>(scr + p.lay.ok);
    L.count = uint32_t(p.count);
    L.items = uint32_t(p.items);
    L.in = d_in;
    L.out = d_out;
    L.tag = d_tag;
    L.status = d_status;
    return L;
}

// env: the messages are envelopes (a seal scatters their header bytes);
// upload: the table holds the keys and goes up here (else the key records are
// on the device already, written by the key agreement kernels)
int gcm_run(bool seal, ecies::Plan &p, const uint8_t *d_in, uint8_t *d_out, uint8_t *d_tag, uint32_t *d_status,
            void *d_scratch, void *stream, bool env = false, bool keep_status = false, bool upload = true) {
    int st = use_device();
    if (st != CHIP_OK) {
        host::secure_wipe(p.table.data(), p.table.size());
        return st;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    if (upload) CHIP_HIP(upload_key_table(p.table, scr, s));
    GcmLaunch L = launch_of(p, scr, d_in, d_out, d_tag, d_status);
    L.keep_status = keep_status;
    hipError_t e = gcm_setup_launch(L, s);
    if (seal) {
        if (e == hipSuccess && env) e = gcm_hdr_launch(L, scr + p.lay.hdrs, true, s);
        if (e == hipSuccess) e = gcm_span_launch(L, gcm::MODE_SEAL, s);
        if (e == hipSuccess) e = gcm_finish_launch(L, true, s);
    } else {
        if (e == hipSuccess) e = gcm_span_launch(L, gcm::MODE_HASH, s);
        if (e == hipSuccess) e = gcm_finish_launch(L, false, s);
        if (e == hipSuccess) e = gcm_span_launch(L, gcm::MODE_CTR, s);
    }
    // the key region goes whatever became of the launches
    const hipError_t w = hipMemsetAsync(scr + p.lay.wipe_from(), 0, p.lay.wipe_len(), s);
    CHIP_HIP(e);
    CHIP_HIP(w);
    return CHIP_OK;
}

// The tail of an envelope call whose keys the device derives: `derived` is what
// became of the uploads and the key kernel; the GCM launches follow if it went
// well, and both key regions are zeroed whatever happened.
int gcm_run_derived(hipError_t derived, bool seal, ecies::Plan &p, const uint8_t *d_in, uint8_t *d_out, uint8_t *d_tag,
                    uint32_t *d_status, void *d_scratch, void *stream, bool keep_status) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    int st = CHIP_OK;
    hipError_t w = hipSuccess;
    if (derived == hipSuccess)
        st = gcm_run(seal, p, d_in, d_out, d_tag, d_status, d_scratch, stream, seal, keep_status, false);
    else
        w = hipMemsetAsync(scr + p.lay.wipe_from(), 0, p.lay.wipe_len(), s);
    const hipError_t wa = agree_wipe_enqueue(scr + p.lay.total, p.count, s);
    CHIP_HIP(derived);
    if (st != CHIP_OK) return st;
    CHIP_HIP(w);
    CHIP_HIP(wa);
    return CHIP_OK;
}

// f(o) for every object on the stage pool's threads and the caller
void for_objects(uint64_t count, const std::function<void(uint64_t)> &f) {
    const int parts = int(std::min<uint64_t>(count, 64));
    host::par_for(parts, [&](int i) {
        for (uint64_t o = uint64_t(i); o < count; o += uint64_t(parts)) f(o);
    });
}

}  // namespace

extern "C" {

int chipe_abi_version(void) { return CHIPE_ABI_VERSION; }

uint64_t chipe_gcm_scratch_len(const uint64_t *n, uint64_t count) { return ecies::gcm_scratch_len(n, count); }

int chipe_gcm_seal_ragged_dev(const uint8_t *keys, const uint8_t *ivs, const uint8_t *d_in, const uint64_t *in_off,
                              const uint64_t *n, uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                              uint8_t *d_tag, void *d_scratch, uint64_t scratch_len, void *stream) {
    if (count == 0) return CHIP_OK;
    ecies::Plan p;
    int st = ecies::plan_gcm(true, keys, ivs, reinterpret_cast<uintptr_t>(d_in), in_off, n, count,
                             reinterpret_cast<uintptr_t>(d_out), out_off, reinterpret_cast<uintptr_t>(d_tag), nullptr,
                             true, reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &p);
    if (st != CHIP_OK) return st;
    return gcm_run(true, p, d_in, d_out, d_tag, nullptr, d_scratch, stream);
}

int chipe_gcm_open_ragged_dev(const uint8_t *keys, const uint8_t *ivs, const uint8_t *d_in, const uint64_t *in_off,
                              const uint64_t *n, uint64_t count, const uint8_t *d_tag, uint8_t *d_out,
                              const uint64_t *out_off, uint32_t *d_status, void *d_scratch, uint64_t scratch_len,
                              void *stream) {
    if (count == 0) return CHIP_OK;
    ecies::Plan p;
    int st = ecies::plan_gcm(false, keys, ivs, reinterpret_cast<uintptr_t>(d_in), in_off, n, count,
                             reinterpret_cast<uintptr_t>(d_out), out_off, reinterpret_cast<uintptr_t>(d_tag), nullptr,
                             d_status != nullptr, reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &p);
    if (st != CHIP_OK) return st;
    return gcm_run(false, p, d_in, d_out, const_cast<uint8_t *>(d_tag), d_status, d_scratch, stream);
}

}  // extern "C"

namespace chip {
namespace api {

int ecies_seal_env(KeySource src, const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                   const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count, uint8_t *d_out,
                   const uint64_t *out_off, void *d_scratch, void *stream) {
    if (count == 0) return CHIP_OK;
    if (!pubkey || !in_off || !n || !out_off || !d_out || !d_scratch || count >= ecies::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> ct_off(count), tag_off(count), env_len(count);
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > ecies::MAX_MSG || out_off[o] > (uint64_t(1) << 53)) return CHIP_ERR_INVALID_ARG;
        ct_off[o] = out_off[o] + ecies::ENV_OVERHEAD;
        tag_off[o] = out_off[o] + ecies::HDR_LEN;
        env_len[o] = n[o] + ecies::ENV_OVERHEAD;
    }
    if (ecies::ranges_overlap(out_off, env_len.data(), count)) return CHIP_ERR_INVALID_ARG;
    ecies::Plan p;
    std::vector<uint8_t> zeros(32 * count, 0);
    int st = ecies::plan_gcm(true, zeros.data(), zeros.data(), reinterpret_cast<uintptr_t>(d_in), in_off, n, count,
                             reinterpret_cast<uintptr_t>(d_out), ct_off.data(), reinterpret_cast<uintptr_t>(d_out),
                             tag_off.data(), true, reinterpret_cast<uintptr_t>(d_scratch), ~uint64_t(0), &p);
    if (st != CHIP_OK) return st;
    uint8_t peer[65];
    st = host::ecies_peer(pubkey, pubkey_len, peer);
    if (st != CHIP_OK) return st;
    if (src == KeySource::Device) {
        // the host's share: the scalars and the nonces; the key records and header slots get their keys on the device
        std::vector<uint8_t> words;
        st = agree_draw(count, [&](uint64_t o) { return inject ? inject[o].ephemeral_sk : nullptr; }, &words);
        const uint8_t none[65] = {0};
        std::vector<uint8_t> ivs(16 * count);  // one RNG call for the batch
        if (st == CHIP_OK && !agree_rand(ivs.data(), ivs.size())) st = CHIP_ERR_ECIES;
        for (uint64_t o = 0; st == CHIP_OK && o < count; ++o) {
            const uint8_t *iv = inject && inject[o].nonce ? inject[o].nonce : ivs.data() + 16 * o;
            ecies::fill_key(p, o, none, iv);
            ecies::fill_hdr(p, o, none, iv);
        }
        if (st == CHIP_OK) st = use_device();
        Ctx *c = nullptr;
        if (st == CHIP_OK) st = ctx_get(&c);
        if (st != CHIP_OK) {
            host::secure_wipe(words.data(), words.size());
            return st;
        }
        hipStream_t s = static_cast<hipStream_t>(stream);
        uint8_t *scr = static_cast<uint8_t *>(d_scratch);
        hipError_t e = h2d(c->stage, scr, p.table.data(), p.lay.upload_len(), s);  // public: no key in it
        if (e == hipSuccess)
            e = agree_seal_enqueue(c, peer, words, count, scr + p.lay.total, scr + p.lay.hdrs, ecies::HDR_PITCH,
                                   scr + p.lay.keys, 48, s);
        else
            host::secure_wipe(words.data(), words.size());
        return gcm_run_derived(e, true, p, d_in, d_out, d_out, nullptr, d_scratch, stream, false);
    }
    st = use_device();
    if (st != CHIP_OK) return st;
    // the key agreement of every object (two scalar multiplications each), then its slots of the table
    std::atomic<int> bad{CHIP_OK};
    for_objects(count, [&](uint64_t o) {
        host::EciesKey k;
        uint8_t iv[16];
        int e = host::ecies_prepare(peer, inject ? inject[o].ephemeral_sk : nullptr, &k);
        if (e == CHIP_OK) {
            if (inject && inject[o].nonce) std::memcpy(iv, inject[o].nonce, 16);
            else if (RAND_bytes(iv, 16) != 1) e = CHIP_ERR_ECIES;
        }
        if (e == CHIP_OK) {
            ecies::fill_key(p, o, k.key, iv);
            ecies::fill_hdr(p, o, k.eph_pub, iv);
        } else {
            bad.store(e);
        }
        host::ecies_key_wipe(&k);
    });
    if (bad.load() != CHIP_OK) {
        host::secure_wipe(p.table.data(), p.table.size());
        return bad.load();
    }
    return gcm_run(true, p, d_in, d_out, d_out, nullptr, d_scratch, stream, true);
}

int ecies_open_env(KeySource src, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in, const uint64_t *in_off,
                   const uint64_t *in_len, uint64_t count, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                   uint32_t *d_status, void *d_scratch, void *stream, bool keep_status, bool check_only) {
    if (count == 0) return CHIP_OK;
    if (!secret_key || !d_in || !in_off || !in_len || !out_off || !out_len || !d_status || !d_scratch ||
        count >= ecies::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> ct_off(count), tag_off(count), ct_len(count);
    std::vector<uint8_t> refused(count, 0);
    for (uint64_t o = 0; o < count; ++o) {
        if (in_off[o] > (uint64_t(1) << 53)) return CHIP_ERR_INVALID_ARG;
        refused[o] = in_len[o] < ecies::ENV_OVERHEAD;
        ct_off[o] = in_off[o] + ecies::ENV_OVERHEAD;
        tag_off[o] = in_off[o] + ecies::HDR_LEN;
        ct_len[o] = refused[o] ? 0 : in_len[o] - ecies::ENV_OVERHEAD;
    }
    ecies::Plan p;
    std::vector<uint8_t> zeros(32 * count, 0);
    int st = ecies::plan_gcm(false, zeros.data(), zeros.data(), reinterpret_cast<uintptr_t>(d_in), ct_off.data(),
                             ct_len.data(), count, reinterpret_cast<uintptr_t>(d_out), out_off,
                             reinterpret_cast<uintptr_t>(d_in), tag_off.data(), true,
                             reinterpret_cast<uintptr_t>(d_scratch), ~uint64_t(0), &p, refused.data());
    if (st != CHIP_OK) return st;
    uint8_t pub[65];
    if (sk_len != 32 || host::ecies_public_key(secret_key, pub) != CHIP_OK) return CHIP_ERR_ECIES;
    for (uint64_t o = 0; o < count; ++o) out_len[o] = ct_len[o];
    if (check_only) return CHIP_OK;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    // the public part of the table, the header bytes of every envelope gathered behind it
    CHIP_HIP(h2d(c->stage, scr, p.table.data(), p.lay.hdrs, s));
    const GcmLaunch G = launch_of(p, scr, d_in, d_out, const_cast<uint8_t *>(d_in), d_status);
    CHIP_HIP(gcm_hdr_launch(G, scr + p.lay.hdrs, false, s));
    if (src == KeySource::Device) {
        // the key kernel reads the header slots, writes the key records and refuses what does not parse
        AgreeOpen A{};
        A.count = uint32_t(count);
        A.eph = scr + p.lay.hdrs;
        A.eph_pitch = ecies::HDR_PITCH;
        A.keys = scr + p.lay.keys;
        A.key_pitch = 48;
        A.refused = scr + p.lay.msgs + offsetof(gcm::Msg, refused);
        A.refused_stride = sizeof(gcm::Msg);
        A.copy_iv = 1;
        const hipError_t e = agree_open_enqueue(secret_key, scr + p.lay.total, A, s);
        return gcm_run_derived(e, false, p, d_in, d_out, const_cast<uint8_t *>(d_in), d_status, d_scratch, stream,
                               keep_status);
    }
    // one copy back: the keys depend on the header bytes, so the call waits here
    std::vector<uint8_t> hdrs(count * ecies::HDR_PITCH);
    CHIP_HIP(d2h(c->stage, hdrs.data(), scr + p.lay.hdrs, hdrs.size(), s));
    for_objects(count, [&](uint64_t o) {
        if (refused[o]) return;
        const uint8_t *h = hdrs.data() + o * ecies::HDR_PITCH;
        uint8_t key[32];
        if (host::ecies_derive_key(secret_key, sk_len, h, key) == CHIP_OK) ecies::fill_key(p, o, key, h + 65);
        else refused[o] = 1;  // an ephemeral key that does not parse
        host::secure_wipe(key, sizeof key);
    });
    for (uint64_t o = 0; o < count; ++o)
        if (refused[o]) ecies::set_refused(p, o);
    return gcm_run(false, p, d_in, d_out, const_cast<uint8_t *>(d_in), d_status, d_scratch, stream, false, keep_status);
}

}  // namespace api
}  // namespace chip

extern "C" {

int chipe_seal_ragged_dev(const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                          const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count, uint8_t *d_out,
                          const uint64_t *out_off, void *d_scratch, void *stream) {
    return ecies_seal_env(KeySource::Host, pubkey, pubkey_len, inject, d_in, in_off, n, count, d_out, out_off, d_scratch,
                          stream);
}

int chipe_open_ragged_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in, const uint64_t *in_off,
                          const uint64_t *in_len, uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                          uint64_t *out_len, uint32_t *d_status, void *d_scratch, void *stream) {
    return ecies_open_env(KeySource::Host, secret_key, sk_len, d_in, in_off, in_len, count, d_out, out_off, out_len,
                          d_status, d_scratch, stream, false, false);
}

}  // extern "C"

// ---- formats 5, 9, 13: Ecies with Bao and / or Zfec, one call ---------------------
namespace {

bool ecies_format(uint8_t f) {
    return f < 16 && (f & CHIP_FORMAT_ECIES) && !(f & CHIP_FORMAT_SNAPPY) && (f & (CHIP_FORMAT_BAO | CHIP_FORMAT_ZFEC));
}

// Scratch of the one-call forms: envelopes (row o of up16(bound[o]) bytes) | GCM scratch (with the agreement's
// behind it when the device derives the keys) | ragged scratch.
struct Regions {
    std::vector<uint64_t> env_off;
    uint64_t gcm = 0, ragged = 0, total = 0;
};
bool regions(KeySource src, uint8_t f12, const uint64_t *plain_bound, const uint64_t *env_bound,
             const uint64_t *ragged_len, uint64_t count, bool decode, Regions *r) {
    r->env_off.resize(count);
    uint64_t at = 0;
    for (uint64_t o = 0; o < count; ++o) {
        r->env_off[o] = at;
        at += ecies::up16(env_bound[o]);
    }
    const uint64_t g = src == KeySource::Device ? chipy_envelope_scratch_len(plain_bound, count)
                                                : ecies::gcm_scratch_len(plain_bound, count);
    const uint64_t x = chipx_ragged_scratch_len(f12, ragged_len, count, decode);
    if (!g) return false;
    r->gcm = at;
    r->ragged = r->gcm + g;
    r->total = ecies::up16(r->ragged + x);
    return true;
}

}  // namespace

namespace chip {
namespace api {

uint64_t ecies_encode_scratch_len(KeySource src, uint8_t format, const uint64_t *n, uint64_t count) {
    if (!ecies_format(format) || !n || count == 0 || count >= ecies::MAX_COUNT) return 0;
    std::vector<uint64_t> env(count);
    for (uint64_t o = 0; o < count; ++o) env[o] = n[o] + ecies::ENV_OVERHEAD;
    Regions r;
    return regions(src, format & 12, n, env.data(), env.data(), count, false, &r) ? r.total : 0;
}

uint64_t ecies_decode_scratch_len(KeySource src, uint8_t format, const uint64_t *in_len, uint64_t count) {
    if (!ecies_format(format) || !in_len || count == 0 || count >= ecies::MAX_COUNT) return 0;
    Regions r;  // a stream is longer than what it decodes to: its length bounds the envelope and the plaintext
    return regions(src, format & 12, in_len, in_len, in_len, count, true, &r) ? r.total : 0;
}

int ecies_encode_env(KeySource src, uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len,
                     const chip_ecies_inject *inject, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n,
                     uint64_t count, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, uint8_t *d_hash,
                     chip_encode_info *info, void *d_scratch, void *stream) {
    if (!ecies_format(format)) return CHIP_ERR_INVALID_ARG;
    if (count == 0) return CHIP_OK;
    if (!pubkey || !in_off || !n || !out_off || !out_len || !d_out || !d_hash || !d_scratch || misaligned16(d_scratch) ||
        count >= ecies::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    const uint8_t f12 = format & 12;
    std::vector<uint64_t> env_len(count);
    for (uint64_t o = 0; o < count; ++o) {
        if (n[o] > (uint64_t(16) << 20) - ecies::ENV_OVERHEAD) return CHIP_ERR_INVALID_ARG;
        env_len[o] = n[o] + ecies::ENV_OVERHEAD;
    }
    Regions r;
    if (!regions(src, f12, n, env_len.data(), env_len.data(), count, false, &r)) return CHIP_ERR_INVALID_ARG;
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    {  // the level-12 half's own checks, before anything is enqueued
        ragged::Plan rp;
        int st = ragged::plan_encode(f12, reinterpret_cast<uintptr_t>(scr), r.env_off.data(), env_len.data(), count,
                                     reinterpret_cast<uintptr_t>(d_out), out_off, out_len, &rp);
        if (st != CHIP_OK) return st;
    }
    int st = ecies_seal_env(src, pubkey, pubkey_len, inject, d_in, in_off, n, count, scr, r.env_off.data(), scr + r.gcm,
                            stream);
    if (st != CHIP_OK) return st;
    st = chipx_encode_ragged_dev(f12, scr, r.env_off.data(), env_len.data(), count, d_out, out_off, out_len, d_hash,
                                 nullptr, scr + r.ragged, stream);
    if (st != CHIP_OK) return st;
    for (uint64_t o = 0; info && o < count; ++o) {  // EncodeInfo of encode() at `format` (encoding.rs:86-171)
        uint64_t zlen, fl;
        st = encode_info_for(format, n[o], env_len[o], 0, env_len[o], &info[o], &zlen, &fl);
        if (st != CHIP_OK) return st;
    }
    return CHIP_OK;
}

int ecies_decode_env(KeySource src, uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                     const uint64_t *in_off, const uint64_t *in_len, uint64_t count, const uint8_t *d_hash,
                     const uint32_t *padding, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                     uint32_t *d_status, void *d_scratch, void *stream) {
    if (!ecies_format(format)) return CHIP_ERR_INVALID_ARG;
    if (count == 0) return CHIP_OK;
    if (!secret_key || !d_in || !in_off || !in_len || !out_off || !out_len || !d_status || !d_scratch ||
        misaligned16(d_scratch) || count >= ecies::MAX_COUNT)
        return CHIP_ERR_INVALID_ARG;
    const uint8_t f12 = format & 12;
    Regions r;
    if (!regions(src, f12, in_len, in_len, in_len, count, true, &r)) return CHIP_ERR_INVALID_ARG;
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    std::vector<uint64_t> env_len(count);
    {  // both halves' checks, before anything is enqueued
        ragged::Plan rp;
        int st = ragged::plan_decode(f12, reinterpret_cast<uintptr_t>(d_in), in_off, in_len, count, padding,
                                     reinterpret_cast<uintptr_t>(scr), r.env_off.data(), env_len.data(), &rp);
        if (st != CHIP_OK) return st;
        if ((f12 & CHIP_FORMAT_BAO) && !d_hash) return CHIP_ERR_HASH_DECODE;
        st = ecies_open_env(src, secret_key, sk_len, scr, r.env_off.data(), env_len.data(), count, d_out, out_off, out_len,
                            d_status, scr + r.gcm, stream, true, true);
        if (st != CHIP_OK) return st;
    }
    int st = chipx_decode_ragged_dev(f12, d_in, in_off, in_len, count, d_hash, padding, scr, r.env_off.data(),
                                     env_len.data(), d_status, scr + r.ragged, stream);
    if (st != CHIP_OK) return st;
    return ecies_open_env(src, secret_key, sk_len, scr, r.env_off.data(), env_len.data(), count, d_out, out_off, out_len,
                          d_status, scr + r.gcm, stream, true, false);
}

}  // namespace api
}  // namespace chip

extern "C" {

uint64_t chipe_encode_scratch_len(uint8_t format, const uint64_t *n, uint64_t count) {
    return ecies_encode_scratch_len(KeySource::Host, format, n, count);
}

uint64_t chipe_decode_scratch_len(uint8_t format, const uint64_t *in_len, uint64_t count) {
    return ecies_decode_scratch_len(KeySource::Host, format, in_len, count);
}

int chipe_encode_ragged_dev(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                            const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                            uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, uint8_t *d_hash,
                            chip_encode_info *info, void *d_scratch, void *stream) {
    return ecies_encode_env(KeySource::Host, format, pubkey, pubkey_len, inject, d_in, in_off, n, count, d_out, out_off,
                            out_len, d_hash, info, d_scratch, stream);
}

int chipe_decode_ragged_dev(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                            const uint64_t *in_off, const uint64_t *in_len, uint64_t count, const uint8_t *d_hash,
                            const uint32_t *padding, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                            uint32_t *d_status, void *d_scratch, void *stream) {
    return ecies_decode_env(KeySource::Host, format, secret_key, sk_len, d_in, in_off, in_len, count, d_hash, padding,
                            d_out, out_off, out_len, d_status, d_scratch, stream);
}

}  // extern "C"
