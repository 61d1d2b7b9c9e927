// api_ragged.cpp — the ragged device batches of include/carbonado_hip_ext.h:
// objects of different lengths in one call.  The checks, the per-object table
// and the layouts are host code in ragged_plan.hpp; this file uploads the
// table into the caller's scratch and enqueues the kernels of
// ragged_kernels.hip behind it.
#include "api_common.hpp"
#include "ragged_kernels.hpp"

using namespace chip;
using namespace chip::api;

namespace {

// the table into d_scratch on s (through the thread's pinned ring: the host
// copy may go once this returns), then the kernels
int enqueue(ragged::Plan &p, uint8_t format, bool decode, uint8_t *d_hash, uint32_t *d_status, void *d_scratch,
            hipStream_t s) {
    Ctx *c;
    int st = ctx_get(&c);
    if (st != CHIP_OK) return st;
    uint8_t *scr = static_cast<uint8_t *>(d_scratch);
    CHIP_HIP(h2d(c->stage, scr, p.table.data(), p.table.size(), s));
    const bool bao = format & CHIP_FORMAT_BAO, zfec = format & CHIP_FORMAT_ZFEC;
    RaggedLaunch L{};
    L.objs = reinterpret_cast<const ragged::Obj *>(scr + p.lay.objs);
    L.groups = reinterpret_cast<const uint32_t *>(scr + p.lay.groups);
    L.blocks = reinterpret_cast<const uint32_t *>(scr + p.lay.blocks);
    L.gcv = scr + p.lay.gcv;
    L.count = p.count;
    L.total_groups = p.total_groups;
    L.parity_blocks = !decode && zfec ? p.total_blocks : 0;
    L.copy_blocks = decode && !bao ? p.total_blocks : 0;
    L.bao = bao;
    L.decode = decode;
    L.hashes = d_hash;
    L.status = d_status;
    CHIP_HIP(ragged_launch(L, s));
    return CHIP_OK;
}

}  // namespace

extern "C" {

int chipx_abi_version(void) { return CHIPX_ABI_VERSION; }

int chipx_ragged_layout(uint8_t format, const uint64_t *n, uint64_t count, uint64_t align, uint64_t stream_offset,
                        uint64_t *out_off, uint64_t *out_len, uint64_t *total) {
    return ragged::layout(format, n, count, align, stream_offset, out_off, out_len, total);
}

uint64_t chipx_ragged_scratch_len(uint8_t format, const uint64_t *len, uint64_t count, int decode) {
    return ragged::scratch_len(format, len, count, decode);
}

int chipx_encode_ragged_dev(uint8_t format, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *n,
                            uint64_t count, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len,
                            uint8_t *d_hash, chip_encode_info *info, void *d_scratch, void *stream) {
    ragged::Plan p;
    int st = ragged::plan_encode(format, reinterpret_cast<uintptr_t>(d_in), in_off, n, count,
                                 reinterpret_cast<uintptr_t>(d_out), out_off, out_len, &p);
    if (st != CHIP_OK) return st;
    if (count == 0) return CHIP_OK;
    if (!d_hash || !d_scratch || misaligned16(d_scratch)) return CHIP_ERR_INVALID_ARG;
    for (uint64_t o = 0; o < count; ++o) {
        chip_encode_info inf;
        uint64_t zlen, fl;
        st = encode_info_for(format, n[o], n[o], 0, 0, &inf, &zlen, &fl);
        if (st != CHIP_OK) return st;
        if (fl != out_len[o]) return CHIP_ERR_INVALID_ARG;  // (the two length formulas agree)
        if (info) info[o] = inf;
    }
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!(format & CHIP_FORMAT_BAO)) CHIP_HIP(hipMemsetAsync(d_hash, 0, 32 * count, s));
    return enqueue(p, format, false, d_hash, nullptr, d_scratch, s);
}

int chipx_decode_ragged_dev(uint8_t format, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len,
                            uint64_t count, const uint8_t *d_hash, const uint32_t *padding, uint8_t *d_out,
                            const uint64_t *out_off, uint64_t *out_len, uint32_t *d_status, void *d_scratch,
                            void *stream) {
    ragged::Plan p;
    int st = ragged::plan_decode(format, reinterpret_cast<uintptr_t>(d_in), in_off, in_len, count, padding,
                                 reinterpret_cast<uintptr_t>(d_out), out_off, out_len, &p);
    if (st != CHIP_OK) return st;
    if (count == 0) return CHIP_OK;
    if ((format & CHIP_FORMAT_BAO) && !d_hash) return CHIP_ERR_HASH_DECODE;
    if (!d_status || !d_scratch || misaligned16(d_scratch)) return CHIP_ERR_INVALID_ARG;
    st = use_device();
    if (st != CHIP_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    CHIP_HIP(hipMemsetAsync(d_status, 0, count * sizeof(uint32_t), s));
    return enqueue(p, format, true, const_cast<uint8_t *>(d_hash), d_status, d_scratch, s);
}

}  // extern "C"
