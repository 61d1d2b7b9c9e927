// snap_kernels.hip — KZ: the snappy framing format (encoding::snap /
// decoding::snap) over a ragged batch of device-resident objects.  The parse,
// the block decoder and the CRC arithmetic are in snap_device.hpp (shared with
// the host check); this file maps waves to blocks, says what a wave does
// together, and stores the results.
//
// Compress: one wave per 64 KiB block (the u16 hash table, up to 32 KiB, in
// LDS; the CRC table takes its place once the parse is done), then one lane
// per object for FrameEncoder's raw rule and the chunk offsets, then one
// workgroup per block to put header and body where they belong.
// Decompress: one lane per stream walks the chunk headers, one wave per slot
// decodes a block in LDS (64 KiB) and stores it, one wave per slot checks the
// CRC of what was stored, one workgroup per stream combines the verdicts.
// Nothing waits on another workgroup, every loop is bounded by a length from
// the table or the block, and no write leaves the object's range whatever
// the bytes are.
#include "snap_kernels.hpp"

#include "carbonado_hip.h"
#include "snap_wave.hpp"

namespace chip {
namespace {

using namespace snap;

// n bytes between global ranges that are apart, by nt threads: 16-B pieces
// where both sides allow, else 4-B stores from unaligned loads, bytes at the ends
__device__ inline void copy_global(uint8_t *dst, const uint8_t *src, size_t n, uint32_t tid, uint32_t nt) {
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(src);
    const size_t unit = ((da ^ sa) & 15) == 0 ? 16 : 4;
    size_t head = size_t(-da) & (unit - 1);
    if (head > n) head = n;
    const size_t body = (n - head) / unit;
    for (size_t i = tid; i < head; i += nt) dst[i] = src[i];
    if (unit == 16) {
        const uint4 *s = reinterpret_cast<const uint4 *>(src + head);
        uint4 *d = reinterpret_cast<uint4 *>(dst + head);
        for (size_t i = tid; i < body; i += nt) d[i] = s[i];
    } else {
        uint32_t *d = reinterpret_cast<uint32_t *>(dst + head);
        for (size_t i = tid; i < body; i += nt) d[i] = load32(src + head + 4 * i);
    }
    for (size_t i = head + body * unit + tid; i < n; i += nt) dst[i] = src[i];
}

// ---------------------------------------------------------------- compress
__global__ __launch_bounds__(64) void snap_block_kernel(SnapLaunch L) {
    __shared__ __attribute__((aligned(16))) uint16_t table[TABLE_MAX];
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const CBlk r = L.blks[b];
    const CObj o = L.objs[r.obj];
    const uint64_t at = uint64_t(r.idx) * MAX_BLOCK;
    const size_t len = size_t(o.n - at < MAX_BLOCK ? o.n - at : MAX_BLOCK);
    const uint8_t *src = L.in + o.in_off + at;
    Wave w{lane};
    const size_t clen = compress_block(w, L.slots + size_t(b) * SLOT_PITCH, src, len, table);
    __syncthreads();
    uint32_t *tab = reinterpret_cast<uint32_t *>(table);  // the parse is done with it
    crc_table_fill(tab, lane);
    __syncthreads();
    const uint32_t crc = wave_crc(tab, src, len, lane);
    if (lane == 0) {
        L.meta[b].clen = uint32_t(clen);
        L.meta[b].crc = crc;
    }
}

__global__ __launch_bounds__(64) void snap_frame_kernel(SnapLaunch L) {
    const uint32_t oi = blockIdx.x * LANES + threadIdx.x;
    if (oi >= L.count) return;
    const CObj o = L.objs[oi];
    uint64_t pos = o.n ? 10 : 0;  // no stream identifier for an empty object
    for (uint32_t k = 0; k < o.nblk; ++k) {
        const uint64_t at = uint64_t(k) * MAX_BLOCK;
        const uint64_t len = o.n - at < MAX_BLOCK ? o.n - at : MAX_BLOCK;
        const uint64_t clen = L.meta[o.blk0 + k].clen;
        const bool raw = clen >= len - len / 8;  // FrameEncoder's rule
        L.meta[o.blk0 + k].off = pos | (raw ? CMETA_RAW : 0);
        pos += 8 + (raw ? len : clen);
    }
    L.out_len[oi] = pos;
}

__global__ __launch_bounds__(256) void snap_gather_kernel(SnapLaunch L) {
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const CBlk r = L.blks[b];
    const CObj o = L.objs[r.obj];
    const CMeta m = L.meta[b];
    const uint64_t at = uint64_t(r.idx) * MAX_BLOCK;
    const uint64_t len = o.n - at < MAX_BLOCK ? o.n - at : MAX_BLOCK;
    const bool raw = (m.off & CMETA_RAW) != 0;
    const uint64_t blen = raw ? len : m.clen;
    uint8_t *stream = L.out + o.out_off;
    uint8_t *chunk = stream + (m.off & ~CMETA_RAW);
    if (r.idx == 0 && tid >= 64 && tid < 74) {
        const uint8_t id[10] = {0xFF, 0x06, 0x00, 0x00, 's', 'N', 'a', 'P', 'p', 'Y'};
        stream[tid - 64] = id[tid - 64];
    }
    if (tid < 8) {
        const uint32_t chunk_len = uint32_t(4 + blen);
        const uint32_t w0 = (raw ? 0x01u : 0x00u) | (chunk_len << 8);
        chunk[tid] = uint8_t(tid < 4 ? w0 >> (8 * tid) : m.crc >> (8 * (tid - 4)));
    }
    copy_global(chunk + 8, raw ? L.in + o.in_off + at : L.slots + size_t(b) * SLOT_PITCH, size_t(blen), tid, 256);
}

// ---------------------------------------------------------------- decompress
__global__ __launch_bounds__(64) void unsnap_walk_kernel(UnsnapLaunch L) {
    const uint32_t oi = blockIdx.x * LANES + threadIdx.x;
    if (oi >= L.count) return;
    const UObj o = L.objs[oi];
    if (L.keep_status && L.status[oi] != 0) {  // an earlier stage's verdict stands
        L.state[oi].status = L.status[oi];
        L.state[oi].need = 0;
        L.out_len[oi] = 0;
        return;
    }
    const uint8_t *in = L.in + o.in_off;
    const uint64_t n = o.in_len;
    uint64_t s = 0, d = 0, chunks = 0;
    bool ident = false, bad = false;
    while (s < n && !bad) {  // snap_walk's first pass, check for check
        if (n - s < 4) {
            bad = true;
            break;
        }
        const uint32_t ty = in[s];
        const uint64_t clen = uint64_t(in[s + 1]) | (uint64_t(in[s + 2]) << 8) | (uint64_t(in[s + 3]) << 16);
        s += 4;
        if (clen > n - s || (!ident && ty != 0xFF)) {
            bad = true;
            break;
        }
        const uint8_t *body = in + s;
        if (ty == 0xFF) {
            const uint8_t id[6] = {'s', 'N', 'a', 'P', 'p', 'Y'};
            bad = clen != 6;
            for (uint32_t i = 0; i < 6 && !bad; ++i) bad = body[i] != id[i];
            ident = true;
        } else if (ty <= 0x01) {
            if (clen < 4) {
                bad = true;
                break;
            }
            const uint32_t want = uint32_t(body[0]) | (uint32_t(body[1]) << 8) | (uint32_t(body[2]) << 16) |
                                  (uint32_t(body[3]) << 24);
            const uint64_t dl = clen - 4;
            uint64_t ulen = dl;
            if (ty == 0x01) {
                bad = dl > MAX_BLOCK;
            } else {
                size_t used;
                bad = !get_varint(body + 4, size_t(dl), &ulen, &used) || ulen > MAX_BLOCK;
            }
            if (bad) break;
            if (chunks < o.nslots) {
                UDesc &ds = L.desc[o.slot0 + chunks];
                ds.src = o.in_off + s + 4;
                ds.out_pos = d;
                ds.dl = uint32_t(dl);
                ds.ulen = uint32_t(ulen);
                ds.want = want;
                ds.kind = ty == 0x01 ? CHUNK_RAW : CHUNK_COMPRESSED;
            }
            ++chunks;
            d += ulen;
        } else if (ty <= 0x7F) {
            bad = true;  // reserved unskippable
            break;
        }  // 0x80..0xFE: padding / reserved skippable
        s += clen;
    }
    uint32_t st = ST_OK;
    uint64_t len = 0;
    if (bad) {
        st = ST_SNAP;
    } else if (d > o.out_cap) {
        st = ST_TOO_SMALL;
        len = d;
    } else if (chunks > o.nslots) {
        st = ST_UNSUPPORTED;
    }
    for (uint64_t k = chunks; k < o.nslots; ++k) L.desc[o.slot0 + k].kind = CHUNK_NONE;
    L.state[oi].status = st;
    L.state[oi].need = d;
    if (st != ST_OK) {  // nothing of this stream is written
        L.status[oi] = st;
        L.out_len[oi] = len;
    }
}

__global__ __launch_bounds__(64) void unsnap_block_kernel(UnsnapLaunch L) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[MAX_BLOCK];
    const uint32_t slot = blockIdx.x, lane = threadIdx.x;
    const uint32_t oi = L.slot_obj[slot];
    uint32_t bad = 0;
    if (L.state[oi].status == ST_OK) {
        const UDesc ds = L.desc[slot];
        uint8_t *out = L.out + L.objs[oi].out_off + ds.out_pos;
        const uint8_t *src = L.in + ds.src;
        if (ds.kind == CHUNK_RAW) {
            copy_global(out, src, ds.dl, lane, LANES);
        } else if (ds.kind == CHUNK_COMPRESSED) {
            Wave w{lane};
            size_t got = 0;
            const bool ok = decode_block(w, src, ds.dl, stage, ds.ulen, &got) && got == ds.ulen;
            __syncthreads();
            if (ok) {  // stored at the end, from LDS: the wave never loads what it stored
                const size_t n = ds.ulen;
                if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) {
                    uint4 *d16 = reinterpret_cast<uint4 *>(out);
                    const uint4 *s16 = reinterpret_cast<const uint4 *>(stage);
                    for (size_t i = lane; i < n / 16; i += LANES) d16[i] = s16[i];
                    for (size_t i = n / 16 * 16 + lane; i < n; i += LANES) out[i] = stage[i];
                } else {
                    for (size_t i = lane; i < n; i += LANES) out[i] = stage[i];
                }
            } else {
                bad = 1;
            }
        }
    }
    if (lane == 0) L.bad[slot] = bad;
}

__global__ __launch_bounds__(64) void unsnap_crc_kernel(UnsnapLaunch L) {
    __shared__ uint32_t tab[256];
    const uint32_t slot = blockIdx.x, lane = threadIdx.x;
    const uint32_t oi = L.slot_obj[slot];
    if (L.state[oi].status != ST_OK) return;
    const UDesc ds = L.desc[slot];
    if (ds.kind == CHUNK_NONE || L.bad[slot]) return;
    crc_table_fill(tab, lane);
    __syncthreads();
    const uint8_t *p = L.out + L.objs[oi].out_off + ds.out_pos;
    const uint32_t crc = wave_crc(tab, p, ds.ulen, lane);
    if (lane == 0 && crc != ds.want) L.bad[slot] = 1;
}

__global__ __launch_bounds__(256) void unsnap_finish_kernel(UnsnapLaunch L) {
    __shared__ uint32_t any;
    const uint32_t oi = blockIdx.x, tid = threadIdx.x;
    const UState st = L.state[oi];
    if (st.status != ST_OK) return;
    const UObj o = L.objs[oi];
    if (tid == 0) any = 0;
    __syncthreads();
    for (uint32_t k = tid; k < o.nslots; k += 256)
        if (L.bad[o.slot0 + k]) any = 1;
    __syncthreads();
    if (any) {  // a block that does not decode, or whose CRC disagrees: no decompressed byte stays
        uint8_t *out = L.out + o.out_off;  // 16-B aligned (checked by the plan)
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (uint64_t i = tid; i < st.need / 16; i += 256) reinterpret_cast<uint4 *>(out)[i] = z;
        for (uint64_t i = st.need / 16 * 16 + tid; i < st.need; i += 256) out[i] = 0;
    }
    if (tid == 0) {
        L.status[oi] = any ? ST_SNAP : ST_OK;
        L.out_len[oi] = any ? 0 : st.need;
    }
}

}  // namespace

hipError_t snap_block_launch(const SnapLaunch &L, hipStream_t stream) {
    if (L.blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(snap_block_kernel, dim3(L.blocks), dim3(64), 0, stream, L);
    return hipGetLastError();
}

hipError_t snap_frame_launch(const SnapLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(snap_frame_kernel, dim3((L.count + 63) / 64), dim3(64), 0, stream, L);
    return hipGetLastError();
}

hipError_t snap_gather_launch(const SnapLaunch &L, hipStream_t stream) {
    if (L.blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(snap_gather_kernel, dim3(L.blocks), dim3(256), 0, stream, L);
    return hipGetLastError();
}

hipError_t unsnap_walk_launch(const UnsnapLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(unsnap_walk_kernel, dim3((L.count + 63) / 64), dim3(64), 0, stream, L);
    return hipGetLastError();
}

hipError_t unsnap_block_launch(const UnsnapLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(unsnap_block_kernel, dim3(L.slots), dim3(64), 0, stream, L);
    return hipGetLastError();
}

hipError_t unsnap_crc_launch(const UnsnapLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(unsnap_crc_kernel, dim3(L.slots), dim3(64), 0, stream, L);
    return hipGetLastError();
}

hipError_t unsnap_finish_launch(const UnsnapLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(unsnap_finish_kernel, dim3(L.count), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace chip
