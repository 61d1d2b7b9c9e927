// api_repair.cpp — the ragged scrub of include/carbonado_hip_repair.h: shard
// verdicts and repair of device-resident Bao|Zfec streams of different
// lengths in one call.  The checks, the scratch layout, the passes and every
// table are host code in repair_plan.hpp; this file uploads the tables into
// the caller's scratch and enqueues KA's checks (audit_kernels.hip), the
// kernels of repair_kernels.hip and KR's encode (ragged_kernels.hip) behind
// them.  chip_scrub_batch_dev (api_scrub.cpp) is the uniform call; the two
// share select_shares and the verdicts behind the mask (stream_rules.hpp).
#include "api_common.hpp"
#include "audit_kernels.hpp"
#include "ragged_kernels.hpp"
#include "repair_kernels.hpp"

using namespace chip;
using namespace chip::api;

namespace {

// The verdict phase on s: the request table and the objects' first requests
// into d_scratch, KA's checks of every request, the fold into d_masks.
int verdicts_enqueue(Ctx *c, uintptr_t d_in, const uint64_t *in_off, const std::vector<uint64_t> &n,
                     const uint32_t *chunk_len, uintptr_t d_hash, uint32_t *d_masks, uint8_t *scr, hipStream_t s) {
    const uint64_t count = n.size();
    const repair::VerdictLayout V(count);
    audit::Plan p;
    std::vector<uint32_t> first;
    int st = repair::plan_verdicts(d_in, in_off, n, chunk_len, d_hash, &p, &first);
    if (st != CHIP_OK) return st;
    uint32_t *rstat = reinterpret_cast<uint32_t *>(scr + V.rstat);
    uint32_t *d_first = reinterpret_cast<uint32_t *>(scr + V.first);
    CHIP_HIP(h2d(c->stage, d_first, first.data(), first.size() * sizeof(uint32_t), s));
    if (p.nreq) {
        CHIP_HIP(h2d(c->stage, scr + V.audit, p.table.data(), p.table.size(), s));
        CHIP_HIP(hipMemsetAsync(rstat, 0, p.nreq * sizeof(uint32_t), s));
        AuditLaunch L = audit_launch_of(p, scr + V.audit);
        L.total_units = 0;  // verdicts only: no content is gathered
        L.proofs = false;
        L.status = rstat;
        CHIP_HIP(audit_verify_launch(L, s));
    }
    CHIP_HIP(repair_fold_launch(rstat, d_first, (uint32_t)count, d_masks, s));
    return CHIP_OK;
}

// One pass on s: its tables, decode, re-encode, compare and commit, and the
// verdicts back (the pass's one synchronisation).
int pass_run(Ctx *c, repair::Pass &p, uint8_t *base, std::vector<uint32_t> *ok, hipStream_t s) {
    CHIP_HIP(h2d(c->stage, base, p.table.data(), p.table.size(), s));
    CHIP_HIP(repair_decode_launch(reinterpret_cast<const repair::Rec *>(base + p.lay.recs),
                                  reinterpret_cast<const uint32_t *>(base + p.lay.blocks), (uint32_t)p.R,
                                  p.total_blocks, s));
    uint8_t *renc = base + p.lay.renc;
    CHIP_HIP(h2d(c->stage, renc, p.enc.table.data(), p.enc.table.size(), s));
    RaggedLaunch L{};
    L.objs = reinterpret_cast<const ragged::Obj *>(renc + p.enc.lay.objs);
    L.groups = reinterpret_cast<const uint32_t *>(renc + p.enc.lay.groups);
    L.blocks = reinterpret_cast<const uint32_t *>(renc + p.enc.lay.blocks);
    L.gcv = renc + p.enc.lay.gcv;
    L.count = p.enc.count;
    L.total_groups = p.enc.total_groups;
    L.parity_blocks = p.enc.total_blocks;
    L.copy_blocks = 0;
    L.bao = true;
    L.decode = false;
    L.hashes = base + p.lay.h2;
    L.status = nullptr;
    CHIP_HIP(ragged_launch(L, s));
    uint32_t *d_ok = reinterpret_cast<uint32_t *>(base + p.lay.ok);
    CHIP_HIP(repair_commit_launch(reinterpret_cast<const repair::Commit *>(base + p.lay.commits),
                                  reinterpret_cast<const uint64_t *>(base + p.lay.units), (uint32_t)p.R, p.total_units,
                                  d_ok, s));
    ok->assign(p.R, 0);
    CHIP_HIP(hipMemcpyAsync(ok->data(), d_ok, p.R * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(hipStreamSynchronize(s));
    return CHIP_OK;
}

}  // namespace

extern "C" {

int chipr_abi_version(void) { return CHIPR_ABI_VERSION; }

uint64_t chipr_scrub_ragged_scratch_len(const uint64_t *in_len, uint64_t count, uint64_t nrepair) {
    return repair::scratch_len(in_len, count, nrepair);
}

int chipr_shard_masks_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                                 const uint8_t *d_hash, const uint32_t *chunk_len, uint32_t *d_masks, void *d_scratch,
                                 uint64_t scratch_len, void *stream) {
    if (count == 0) return CHIP_OK;
    std::vector<uint64_t> n;
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_in), hash = reinterpret_cast<uintptr_t>(d_hash);
    int st = repair::check_args(false, in, in_off, in_len, count, hash, nullptr, chunk_len, 0, nullptr, d_masks,
                                reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &n);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    return verdicts_enqueue(c, in, in_off, n, chunk_len, hash, d_masks, static_cast<uint8_t *>(d_scratch),
                            static_cast<hipStream_t>(stream));
}

int chipr_scrub_ragged_dev(const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint64_t count,
                           const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len, uint8_t *d_out,
                           const uint64_t *out_off, int32_t *status, void *d_scratch, uint64_t scratch_len,
                           void *stream) {
    if (count == 0) return CHIP_OK;
    std::vector<uint64_t> n;
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_in), hash = reinterpret_cast<uintptr_t>(d_hash);
    const uintptr_t out = reinterpret_cast<uintptr_t>(d_out);
    int st = repair::check_args(true, in, in_off, in_len, count, hash, padding, chunk_len, out, out_off, status,
                                reinterpret_cast<uintptr_t>(d_scratch), scratch_len, &n);
    if (st != CHIP_OK) return st;
    st = use_device();
    if (st != CHIP_OK) return st;
    Ctx *c;
    st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    const repair::VerdictLayout V(count);
    uint32_t *d_masks = reinterpret_cast<uint32_t *>(scr + V.masks);
    st = verdicts_enqueue(c, in, in_off, n, chunk_len, hash, d_masks, scr, s);
    if (st != CHIP_OK) return st;
    std::vector<uint32_t> masks(count);
    CHIP_HIP(hipMemcpyAsync(masks.data(), d_masks, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(hipStreamSynchronize(s));

    // each stream's status, or its place among the repairs (decoding.rs:168-187)
    std::vector<repair::Repair> reps;
    for (uint64_t o = 0; o < count; ++o) {
        const int pre = repair::pre_status(in_len[o], n[o], chunk_len[o], padding[o], masks[o]);
        status[o] = pre;
        if (pre >= 0) continue;
        uint32_t good[CHIP_FEC_M], ngood = 0;
        for (uint32_t i = 0; i < CHIP_FEC_M; ++i)
            if (masks[o] >> i & 1) good[ngood++] = i;
        std::vector<uint32_t> pos;
        if (select_shares(CHIP_FEC_K, CHIP_FEC_M, good, ngood, &pos) != CHIP_OK) {
            status[o] = CHIP_ERR_ZFEC;
            continue;
        }
        repair::Repair r{o, n[o], padding[o], {}};
        for (uint32_t k = 0; k < CHIP_FEC_K; ++k) r.sel[k] = (uint8_t)good[pos[k]];
        reps.push_back(r);
    }
    if (reps.empty()) return CHIP_OK;

    uint8_t *base = scr + V.end;
    std::vector<uint32_t> ok;
    for (const auto &range : repair::pack(reps, scratch_len - V.end)) {
        repair::Pass p;
        st = repair::plan_pass(reps.data() + range.first, range.second - range.first,
                               reinterpret_cast<uintptr_t>(base), in, in_off, out, out_off, hash, &p);
        if (st == CHIP_OK) st = pass_run(c, p, base, &ok, s);
        if (st != CHIP_OK) return st;
        for (size_t j = range.first; j < range.second; ++j)  // decoding.rs:205-207
            status[reps[j].obj] = ok[j - range.first] ? CHIP_OK : CHIP_ERR_INVALID_SCRUBBED_HASH;
    }
    return CHIP_OK;
}

}  // extern "C"
