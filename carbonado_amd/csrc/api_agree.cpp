// api_agree.cpp — the calls of include/carbonado_hip_agree.h.  The checks, the
// scratch layout and the table conversions are host code in agree_plan.hpp;
// this file keeps the comb table of G on the device (built once per process),
// builds and uploads the receiver's, uploads the scalars through the
// pinned-and-wiped path of key_upload.hpp, enqueues the kernels of
// agree_kernels.hip and, last, the memset that zeroes the key region.  The
// envelope and one-call forms are those of api_ecies.cpp with the keys taken
// from here (api_agree.hpp).
#include "api_agree.hpp"

#include <openssl/rand.h>

#include <mutex>

#include "agree_kernels.hpp"
#include "agree_plan.hpp"
#include "api_kread.hpp"
#include "cread_kernels.hpp"
#include "ecies_plan.hpp"
#include "key_upload.hpp"

using namespace chip;
using namespace chip::api;

namespace {

// The comb table of G: a constant, made once per process from k1::gtable() and
// kept in device memory.  One pointer per PROCESS, not per device: the library
// runs one GPU per process (chip_init).  The first seal of a process that needs
// it BLOCKS: hipMalloc and a synchronous hipMemcpy on the null stream.
struct GTable {
    std::mutex mu;
    uint32_t *d = nullptr;
};
GTable g_gtab;

hipError_t gtab_get(const uint32_t **out) {
    std::lock_guard<std::mutex> lk(g_gtab.mu);
    if (!g_gtab.d) {
        std::vector<uint32_t> w(agree::COMB_WORDS);
        agree::fill_comb(k1::gtable(), w.data());
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, w.size() * 4);
        if (e != hipSuccess) return e;
        e = hipMemcpy(p, w.data(), w.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
        g_gtab.d = static_cast<uint32_t *>(p);
    }
    *out = g_gtab.d;
    return hipSuccess;
}

// The comb table of the receiver a thread saw last (public data; ~0.3 ms to build).
struct PeerTable {
    bool valid = false;
    uint8_t key[64];
    std::vector<uint32_t> words;
};
thread_local PeerTable t_peer;

const std::vector<uint32_t> &peer_table(const uint8_t peer[65]) {
    PeerTable &t = t_peer;
    if (!t.valid || std::memcmp(t.key, peer + 1, 64) != 0) {
        k1::Fe x, y;
        (void)k1::parse_full(peer, x, y);  // (checked by host::ecies_peer)
        auto comb = std::make_unique<k1::CombTable>(x, y);
        t.words.resize(agree::COMB_WORDS);
        agree::fill_comb(*comb, t.words.data());
        std::memcpy(t.key, peer + 1, 64);
        t.valid = true;
    }
    return t.words;
}

// Scratch of chipy_key_table_dev over ns streams: [header slots, 96 B each | content lengths | status, used,
// vouch and shorter words | the requests | the planned vouched read's scratch | the agreement's scratch].
struct KeyTableScratch {
    uint64_t hdrs = 0, clen = 0, status = 0, used = 0, vouch = 0, shorter = 0, req_stream = 0, start = 0, len = 0,
             read = 0, agree = 0, total = 0;
    bool ok = false;
    KeyTableScratch(const chipq_table_info *info, uint64_t ns) {
        const uint64_t r = qread::scratch_len(info, ns, ecies::HDR_LEN, true), a = agree::keys_scratch_len(ns);
        if (!r || !a) return;
        const uint64_t w = rules::up16(4 * ns);
        clen = ns * ecies::HDR_PITCH;
        status = clen + rules::up16(8 * ns);
        used = status + w;
        vouch = used + w;
        shorter = vouch + w;
        req_stream = shorter + w;
        start = req_stream + w;
        len = start + rules::up16(8 * ns);
        read = len + rules::up16(8 * ns);
        agree = read + r;
        total = agree + a;
        ok = true;
    }
};

}  // namespace

namespace chip {
namespace api {

bool agree_rand(uint8_t *p, size_t n) {
    for (size_t at = 0; at < n;) {
        const size_t step = std::min<size_t>(n - at, size_t(1) << 30);
        if (RAND_bytes(p + at, int(step)) != 1) return false;
        at += step;
    }
    return true;
}

int agree_draw(uint64_t count, const std::function<const uint8_t *(uint64_t)> &injected, std::vector<uint8_t> *words) {
    words->assign(32 * count, 0);
    std::vector<uint8_t> drawn;  // one RNG call for the batch (a call per object costs more than the bytes)
    int st = CHIP_OK;
    for (uint64_t o = 0; o < count && st == CHIP_OK; ++o) {
        uint8_t sk[32];
        const uint8_t *given = injected(o);
        if (given) {
            std::memcpy(sk, given, 32);
            if (!agree::scalar_ok(sk)) st = CHIP_ERR_ECIES;
        } else {
            if (drawn.empty()) {
                drawn.resize(32 * (count - o));
                if (!agree_rand(drawn.data(), drawn.size())) st = CHIP_ERR_ECIES;
            }
            std::memcpy(sk, drawn.data() + drawn.size() - 32 * (count - o), 32);
            while (st == CHIP_OK && !agree::scalar_ok(sk))  // SecretKey::random: rejection-sample a valid scalar
                if (RAND_bytes(sk, 32) != 1) st = CHIP_ERR_ECIES;
        }
        if (st == CHIP_OK) agree::scalar_words(sk, words->data() + 32 * o);
        host::secure_wipe(sk, sizeof sk);
    }
    if (!drawn.empty()) host::secure_wipe(drawn.data(), drawn.size());
    if (st != CHIP_OK) host::secure_wipe(words->data(), words->size());
    return st;
}

hipError_t agree_seal_enqueue(Ctx *c, const uint8_t peer[65], std::vector<uint8_t> &words, uint64_t count, uint8_t *ascr,
                              uint8_t *pub, uint64_t pub_pitch, uint8_t *keys, uint64_t key_pitch, hipStream_t s) {
    const agree::KeysLayout lay = agree::keys_layout(count);
    AgreeSeal L{};
    hipError_t e = gtab_get(&L.gtab);
    if (e == hipSuccess) {
        const std::vector<uint32_t> &pt = peer_table(peer);
        e = h2d(c->stage, ascr + lay.ptab, pt.data(), pt.size() * 4, s);
    }
    if (e != hipSuccess) {
        host::secure_wipe(words.data(), words.size());
        return e;
    }
    e = upload_key_table(words, ascr + lay.sk, s);
    if (e != hipSuccess) return e;
    L.ptab = reinterpret_cast<const uint32_t *>(ascr + lay.ptab);
    L.sk = reinterpret_cast<const uint32_t *>(ascr + lay.sk);
    L.count = uint32_t(count);
    L.pub = pub;
    L.pub_pitch = pub_pitch;
    L.keys = keys;
    L.key_pitch = key_pitch;
    return agree_seal_launch(L, s);
}

hipError_t agree_open_enqueue(const uint8_t secret[32], uint8_t *ascr, AgreeOpen L, hipStream_t s) {
    const agree::KeysLayout lay = agree::keys_layout(L.count);
    std::vector<uint8_t> words(32);
    agree::scalar_words(secret, words.data());
    hipError_t e = upload_key_table(words, ascr + lay.sk, s);
    if (e != hipSuccess) return e;
    L.sk = reinterpret_cast<const uint32_t *>(ascr + lay.sk);
    L.vtab = reinterpret_cast<uint32_t *>(ascr + lay.vtab);
    return agree_open_launch(L, s);
}

hipError_t agree_wipe_enqueue(uint8_t *ascr, uint64_t count, hipStream_t s) {
    const agree::KeysLayout lay = agree::keys_layout(count);
    return hipMemsetAsync(ascr + lay.wipe_from(), 0, lay.wipe_len(), s);
}

}  // namespace api
}  // namespace chip

extern "C" {

int chipy_abi_version(void) { return CHIPY_ABI_VERSION; }

uint64_t chipy_keys_scratch_len(uint64_t count) { return agree::keys_scratch_len(count); }

int chipy_seal_keys_dev(const uint8_t *pubkey, uint64_t pubkey_len, const uint8_t *eph_sk, uint64_t count, uint8_t *d_pub,
                        uint64_t pub_pitch, uint8_t *d_keys, uint64_t key_pitch, void *d_scratch, uint64_t scratch_len,
                        void *stream) {
    if (count == 0) return CHIP_OK;
    int st = agree::check_seal_keys(pubkey && d_pub && d_keys && d_scratch, count, pub_pitch, key_pitch,
                                    reinterpret_cast<uintptr_t>(d_scratch), scratch_len);
    if (st != CHIP_OK) return st;
    uint8_t peer[65];
    st = host::ecies_peer(pubkey, pubkey_len, peer);
    if (st != CHIP_OK) return st;
    std::vector<uint8_t> words;
    st = agree_draw(count, [&](uint64_t o) { return eph_sk ? eph_sk + 32 * o : nullptr; }, &words);
    if (st != CHIP_OK) return st;
    st = use_device();
    Ctx *c = nullptr;
    if (st == CHIP_OK) st = ctx_get(&c);
    if (st != CHIP_OK) {
        host::secure_wipe(words.data(), words.size());
        return st;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    const hipError_t e = agree_seal_enqueue(c, peer, words, count, scr, d_pub, pub_pitch, d_keys, key_pitch, s);
    const hipError_t w = agree_wipe_enqueue(scr, count, s);  // the key region goes whatever became of the launch
    CHIP_HIP(e);
    CHIP_HIP(w);
    return CHIP_OK;
}

int chipy_open_keys_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_eph, uint64_t eph_pitch,
                        uint64_t count, uint8_t *d_keys, uint64_t key_pitch, uint32_t *d_status, void *d_scratch,
                        uint64_t scratch_len, void *stream) {
    if (count == 0) return CHIP_OK;
    int st = agree::check_open_keys(secret_key && d_eph && d_keys && d_status && d_scratch, count, eph_pitch, key_pitch,
                                    reinterpret_cast<uintptr_t>(d_scratch), scratch_len);
    if (st != CHIP_OK) return st;
    if (sk_len != 32 || !agree::scalar_ok(secret_key)) return CHIP_ERR_ECIES;
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    AgreeOpen A{};
    A.count = uint32_t(count);
    A.eph = d_eph;
    A.eph_pitch = eph_pitch;
    A.keys = d_keys;
    A.key_pitch = key_pitch;
    A.status = d_status;
    const hipError_t e = agree_open_enqueue(secret_key, scr, A, s);
    const hipError_t w = agree_wipe_enqueue(scr, count, s);
    CHIP_HIP(e);
    CHIP_HIP(w);
    return CHIP_OK;
}

uint64_t chipy_key_table_scratch_len(const chipq_table_info *info) {
    if (!info || info->nstreams == 0 || info->nstreams >= agree::MAX_COUNT) return 0;
    const KeyTableScratch lay(info, info->nstreams);
    return lay.ok ? lay.total : 0;
}

int chipy_key_table_dev(const void *d_table, const chipq_table_info *info, const uint8_t *secret_key, uint64_t sk_len,
                        void *d_keytab, uint64_t keytab_len, void *d_scratch, uint64_t scratch_len, void *stream) {
    if (!info) return CHIP_ERR_INVALID_ARG;
    const uint64_t ns = info->nstreams;
    if (ns == 0) return CHIP_OK;
    if (!d_table || !secret_key || !d_keytab || !d_scratch || ns >= agree::MAX_COUNT || misaligned16(d_table) ||
        misaligned16(d_keytab) || misaligned16(d_scratch) || keytab_len < kread::table_len(ns))
        return CHIP_ERR_INVALID_ARG;
    const KeyTableScratch lay(info, ns);
    if (!lay.ok || scratch_len < lay.total) return CHIP_ERR_INVALID_ARG;
    if (sk_len != 32 || !agree::scalar_ok(secret_key)) return CHIP_ERR_ECIES;
    int st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch), *tab = static_cast<uint8_t *>(d_keytab);
    const kread::TableLayout tl(ns);
    auto words = [&](uint64_t off) { return reinterpret_cast<uint32_t *>(scr + off); };
    auto longs = [&](uint64_t off) { return reinterpret_cast<uint64_t *>(scr + off); };
    // the requests, written by a kernel: envelope bytes [0, 81) of every stream
    AgreeRequests R{d_table, uint32_t(ns), words(lay.req_stream), longs(lay.start), longs(lay.len), words(lay.shorter)};
    CHIP_HIP(agree_requests_launch(R, s));
    // a strict vouched planned read of them into the header slots: only bytes hashed against the root
    st = read_planned(QreadCall{d_table, info, R.req_stream, R.start, R.len, ns, ecies::HDR_LEN, scr + lay.hdrs,
                                ecies::HDR_PITCH, longs(lay.clen), words(lay.status), words(lay.used), words(lay.vouch),
                                CHIPV_STRICT, scr + lay.read, lay.agree - lay.read, stream},
                      true);
    if (st != CHIP_OK) return st;
    // key || iv and the key_status word of every stream into the table's staging part, then the table's own setup
    uint32_t *key_status = reinterpret_cast<uint32_t *>(tab + tl.status);
    CHIP_HIP(hipMemsetAsync(tab + tl.status, 0, tl.raw - tl.status, s));  // (the words' padding up to the raw records)
    AgreeOpen A{};
    A.count = uint32_t(ns);
    A.eph = scr + lay.hdrs;
    A.eph_pitch = ecies::HDR_PITCH;
    A.keys = tab + tl.raw;
    A.key_pitch = cread::RAW_KEY;
    A.status = key_status;
    A.copy_iv = 1;
    A.gate = words(lay.status);
    A.shorter = R.shorter;
    hipError_t e = agree_open_enqueue(secret_key, scr + lay.agree, A, s);
    CtrLaunch L{};
    L.rawkeys = tab + tl.raw;
    L.km = reinterpret_cast<cread::CtrKey *>(tab + tl.km);
    L.keys_used = uint32_t(ns);
    if (e == hipSuccess) e = ctr_setup_launch(L, s);
    // the raw records and the secret go whatever became of the launches
    const hipError_t w = kread_table_finish_launch(L.km, key_status, tab + tl.raw, uint32_t(ns), s);
    const hipError_t wa = agree_wipe_enqueue(scr + lay.agree, ns, s);
    CHIP_HIP(e);
    CHIP_HIP(w);
    CHIP_HIP(wa);
    return CHIP_OK;
}

uint64_t chipy_envelope_scratch_len(const uint64_t *n, uint64_t count) {
    const uint64_t g = chipe_gcm_scratch_len(n, count), a = agree::keys_scratch_len(count);
    return g && a ? g + a : 0;
}

int chipy_seal_ragged_dev(const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject, const uint8_t *d_in,
                          const uint64_t *in_off, const uint64_t *n, uint64_t count, uint8_t *d_out,
                          const uint64_t *out_off, void *d_scratch, void *stream) {
    return ecies_seal_env(KeySource::Device, pubkey, pubkey_len, inject, d_in, in_off, n, count, d_out, out_off,
                          d_scratch, stream);
}

int chipy_open_ragged_dev(const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in, const uint64_t *in_off,
                          const uint64_t *in_len, uint64_t count, uint8_t *d_out, const uint64_t *out_off,
                          uint64_t *out_len, uint32_t *d_status, void *d_scratch, void *stream) {
    return ecies_open_env(KeySource::Device, secret_key, sk_len, d_in, in_off, in_len, count, d_out, out_off, out_len,
                          d_status, d_scratch, stream, false, false);
}

uint64_t chipy_encode_scratch_len(uint8_t format, const uint64_t *n, uint64_t count) {
    return ecies_encode_scratch_len(KeySource::Device, format, n, count);
}

uint64_t chipy_decode_scratch_len(uint8_t format, const uint64_t *in_len, uint64_t count) {
    return ecies_decode_scratch_len(KeySource::Device, format, in_len, count);
}

int chipy_encode_ragged_dev(uint8_t format, const uint8_t *pubkey, uint64_t pubkey_len, const chip_ecies_inject *inject,
                            const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n, uint64_t count,
                            uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, uint8_t *d_hash,
                            chip_encode_info *info, void *d_scratch, void *stream) {
    return ecies_encode_env(KeySource::Device, format, pubkey, pubkey_len, inject, d_in, in_off, n, count, d_out, out_off,
                            out_len, d_hash, info, d_scratch, stream);
}

int chipy_decode_ragged_dev(uint8_t format, const uint8_t *secret_key, uint64_t sk_len, const uint8_t *d_in,
                            const uint64_t *in_off, const uint64_t *in_len, uint64_t count, const uint8_t *d_hash,
                            const uint32_t *padding, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                            uint32_t *d_status, void *d_scratch, void *stream) {
    return ecies_decode_env(KeySource::Device, format, secret_key, sk_len, d_in, in_off, in_len, count, d_hash, padding,
                            d_out, out_off, out_len, d_status, d_scratch, stream);
}

}  // extern "C"
