// hostbatch_plan.hpp — the planning arithmetic of encode() and decode() from
// host memory (api_encode.cpp, api_decode.cpp, api_single.cpp): the part of a
// stream the host makes itself, how a batch is cut into slices, the sizes an
// encode's buffers are bound by, EncodeInfo, and the device-stage geometry of
// an encoded object.  Pure host code without a HIP type in it:
// tests/hostbatch_plan_check.cpp compiles it alone under a sanitizer.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "audit_nodes.hpp"
#include "host_stages.hpp"
#include "stream_rules.hpp"

namespace chip {
namespace hostbatch {

// ---- the host-made region of a stream ------------------------------------------
// A stream of zl content bytes (N chunks) whose first `nh` chunks the host
// holds: their slots, the parent-node runs between them (dst: stream offset,
// src: offset in the device's compact node buffer) and the end t0 of that
// region.  encode() at Zfec|Bao from host memory is (1024 N, N / 2): the data
// shards are the zero-padded input, so the header and the chunks [0, nh) are
// the host's, the device gathers the region's nodes compactly (bao_data_nodes,
// or KM for one object) and only they and the tail [t0, end) cross PCIe.
struct HostGeo {
    uint64_t N = 0, nh = 0, zl = 0, t0 = 8, nbytes = 0;  // nbytes: compact node bytes
    std::vector<uint64_t> coff;  // slots of chunks [0, nh), then (tail) of chunks [nh, N)
    struct Run {
        uint64_t dst, src, len;
    };
    std::vector<Run> runs;   // the nodes in front of t0: stream offset, compact offset, bytes
    std::vector<Run> truns;  // the nodes past t0 (tail only): stream offset, -, bytes
};

// tail: also the slots of the chunks [nh, N) and the node runs between them
inline HostGeo host_geo(uint64_t zl, uint64_t nh, bool tail = true) {
    HostGeo g;
    g.zl = zl;
    g.N = rules::chunks(zl);
    g.nh = nh;
    const uint64_t nc = tail ? g.N : nh;
    g.coff.resize(nc);
    // chunk 0 at audit::stream_off; chunk i + 1 behind chunk i's slot and the parents whose
    // leftmost chunk it is (audit_nodes.hpp: stream_off(s + 1) - stream_off(s) = 1024 + 64 c(s + 1)),
    // O(1) a chunk: stream_off itself per chunk cost a 16 MiB batch call 0.4 ms
    uint64_t prev_end = 8, off = audit::stream_off(0, 0, g.N);
    for (uint64_t i = 0; i < nc; ++i) {
        if (i == nh) g.t0 = prev_end;
        if (i) off += 1024 + 64 * (uint64_t)audit::parents_at(i, g.N);
        g.coff[i] = off;
        if (g.coff[i] > prev_end) {
            const uint64_t len = g.coff[i] - prev_end;
            if (i < nh) g.runs.push_back({prev_end, g.nbytes, len}), g.nbytes += len;
            else g.truns.push_back({prev_end, 0, len});
        }
        prev_end = g.coff[i] + audit::chunk_len(i, zl);
    }
    if (nc == nh) g.t0 = prev_end;
    return g;
}

// ---- slices ---------------------------------------------------------------------
// A host batch runs `nslices` slices of S objects (the last one shorter)
// through `nslots` pipeline slots, the host work of a slice on T threads.
struct Slices {
    uint32_t nslots, T;
    uint64_t S, nslices;
};

// nslots 1..8 (0: 3), slice_bytes (0: 256 MiB) over the largest object,
// host_threads (0: the hardware's, hw_threads) capped at 64.  round_to_threads
// (host work per object): a slice of at least half as many objects as host
// threads is rounded up to a multiple of them (equal shares).  count >= 1.
inline Slices plan_slices(uint32_t nslots, uint64_t slice_bytes, uint32_t host_threads, uint32_t hw_threads,
                          uint64_t max_bytes, uint64_t count, bool round_to_threads) {
    Slices p;
    p.nslots = nslots < 1 ? 3 : (nslots > 8 ? 8 : nslots);
    if (slice_bytes == 0) slice_bytes = 256ull << 20;
    p.T = std::min<uint32_t>(host_threads ? host_threads : std::max(1u, hw_threads), 64);
    p.S = std::max<uint64_t>(1, slice_bytes / (max_bytes ? max_bytes : 1));
    if (round_to_threads && p.S >= (p.T + 1) / 2) p.S = rules::up(p.S, p.T);
    p.S = std::min(p.S, count);
    p.nslices = (count + p.S - 1) / p.S;
    return p;
}

// ---- encode ---------------------------------------------------------------------
inline bool has_host_stages(uint8_t format) { return format & (CHIP_FORMAT_ECIES | CHIP_FORMAT_SNAPPY); }

// bound of the host stages' output for an n-byte input
inline uint64_t host_stage_max(uint8_t format, uint64_t n) {
    uint64_t m = (format & CHIP_FORMAT_SNAPPY) ? host::snap_max_len(n) : n;
    if (format & CHIP_FORMAT_ECIES) m += host::ECIES_OVERHEAD;
    return m;
}

// EncodeInfo of encode() (encoding.rs:86-171): `input_len` is the caller's
// input, `cur` the length entering zfec (after snap/ecies), bc/be the
// snap/ecies output lengths (0 when the stage is off, encoding.rs:101-115).
inline int encode_info_for(uint8_t format, uint64_t input_len, uint64_t cur, uint64_t bc, uint64_t be,
                           chip_encode_info *inf, uint64_t *zlen, uint64_t *final_len) {
    std::memset(inf, 0, sizeof *inf);
    inf->input_len = (uint32_t)input_len;  // encoding.rs:87 (as u32)
    inf->bytes_compressed = (uint32_t)bc;
    inf->bytes_encrypted = (uint32_t)be;
    const bool zfec = format & CHIP_FORMAT_ZFEC, bao = format & CHIP_FORMAT_BAO;
    uint64_t cur_len = cur;
    if (zfec) {
        const rules::Pad p = rules::calc_pad(cur, CHIP_FEC_K);
        inf->padding_len = p.pad;
        inf->chunk_len = (uint32_t)p.C;
        cur_len = (uint64_t)CHIP_FEC_M * p.C;
        inf->bytes_ecc = (uint32_t)cur_len;                                        // encoding.rs:123
        inf->verifiable_slice_count = (uint16_t)(inf->bytes_ecc / CHIP_SLICE_LEN);  // encoding.rs:124
        if (inf->verifiable_slice_count % 8 != 0) return CHIP_ERR_INVALID_VERIFIABLE_SLICE_COUNT;
        inf->chunk_slice_count = inf->verifiable_slice_count / 8;                  // encoding.rs:130
    }
    const uint64_t fl = bao ? rules::bao_len(cur_len) : cur_len;
    if (bao) inf->bytes_verifiable = (uint32_t)fl;
    inf->compression_factor = (float)inf->bytes_compressed / (float)inf->input_len;    // encoding.rs:150
    inf->amplification_factor = (float)inf->bytes_verifiable / (float)inf->input_len;  // encoding.rs:151
    inf->output_len = (uint32_t)fl;
    *zlen = cur_len;
    *final_len = fl;
    return CHIP_OK;
}

// chunk count of the bao stream of a Zfec|Bao object whose host stages left len bytes
inline uint64_t split_chunks(uint64_t len) { return (uint64_t)CHIP_FEC_M * rules::calc_pad(len, CHIP_FEC_K).C / 1024; }

// What a host batch of n-byte objects sizes its buffers by: exact without host
// stages (st: encode_info_for's, inf: every object's EncodeInfo), bounds with
// them (st OK: the slice-count check is each object's own, a smaller output
// may still pass it).
struct EncodeBounds {
    int st = CHIP_OK;
    uint64_t h_max = 0, zlen_max = 0, final_max = 0;  // entering zfec, leaving it, the encoded object
    chip_encode_info inf;
};
inline EncodeBounds encode_bounds(uint8_t format, uint64_t n) {
    EncodeBounds b;
    const bool hs = has_host_stages(format);
    b.h_max = hs ? host_stage_max(format, n) : n;
    b.st = encode_info_for(format, n, b.h_max, 0, 0, &b.inf, &b.zlen_max, &b.final_max);
    if (hs) b.st = CHIP_OK;
    b.zlen_max = (format & CHIP_FORMAT_ZFEC) ? (uint64_t)CHIP_FEC_M * rules::calc_pad(b.h_max, CHIP_FEC_K).C : b.h_max;
    b.final_max = (format & CHIP_FORMAT_BAO) ? rules::bao_len(b.zlen_max) : b.zlen_max;
    return b;
}

// ---- decode ---------------------------------------------------------------------
// content length of the bao stream at enc[0, len), read from its header
inline int bao_header(const uint8_t *enc, uint64_t len, uint64_t *n) {
    if (len < 8) return CHIP_ERR_BAO_TRUNCATED;
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)enc[i] << (8 * i);
    // a stream shorter than its header implies is truncated (also guards overflow)
    if (v > len || rules::bao_len(v) > len) return CHIP_ERR_BAO_TRUNCATED;
    *n = v;
    return CHIP_OK;
}

// device-stage geometry of one encoded object (decoding.rs:80-99)
struct DecGeom {
    int st = CHIP_OK;
    uint64_t blen = 0;  // bytes entering zfec (bao content length, or the input length)
    uint64_t olen = 0;  // bytes leaving zfec (k*C - padding, or blen)
};
inline DecGeom dec_geom(uint8_t format, const uint8_t *in, uint64_t n, uint32_t padding) {
    DecGeom g;
    g.blen = n;
    if (format & CHIP_FORMAT_BAO) {
        g.st = bao_header(in, n, &g.blen);
        if (g.st != CHIP_OK) return g;
    }
    g.olen = g.blen;
    if (format & CHIP_FORMAT_ZFEC) {
        if (g.blen % CHIP_FEC_M) g.st = CHIP_ERR_UNEVEN_ZFEC_CHUNKS;  // decoding.rs:39-41
        else if (padding > CHIP_FEC_K * (g.blen / CHIP_FEC_M)) g.st = CHIP_ERR_ZFEC;
        else g.olen = CHIP_FEC_K * (g.blen / CHIP_FEC_M) - padding;
    }
    return g;
}

}  // namespace hostbatch
}  // namespace chip
