// snap_device.hpp — the snappy block compressor, the block decoder and the
// CRC-32C of the framing format as __host__ __device__ code: one text for the
// kernels of snap_kernels.hip (KZ) and for the host check
// (tests/snap_device_check.cpp), as gcm_device.hpp is for KE.
//
// The parse is encode_block / compress_raw / decompress_raw of host_snap.cpp
// restated step for step; what a wave does together is behind a small policy
// type W so that the same text runs on one host thread:
//   w.copy(dst, src, n)       n bytes, ranges apart, any order
//   w.match(src, a, b, n)     largest m with src[a + i] == src[b + i] for i < m, b + m <= n   (a < b)
//   w.zero16(t, n)            n uint16 entries to zero
//   w.put(p, v)               one byte, once
//   w.rep(stage, d, off, c)   stage[d + i] = stage[d - off + i % off] for i < c <= 64 (reads before writes)
//   w.sync()                  what the wave wrote is what every lane reads next
//   w.uni(x)                  a value every lane holds alike (a hint: scalar registers on the device)
// The result never depends on the order inside these, so the bytes are the
// host's.  No secret is involved: tables and data-dependent branches are fine.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SNAP_HD __host__ __device__ inline
#else
#define SNAP_HD inline
#endif

namespace chip {
namespace snap {

constexpr uint32_t MAX_BLOCK = 65536;                                   // FrameEncoder's block
constexpr uint32_t MAX_COMPRESS_BLOCK = 32 + MAX_BLOCK + MAX_BLOCK / 6;  // max_compress_len(64 KiB)
constexpr uint32_t SLOT_PITCH = (MAX_COMPRESS_BLOCK + 15) / 16 * 16;     // a block's private slot in the scratch
constexpr uint32_t LANES = 64;
constexpr uint32_t TABLE_MAX = 16384;  // u16 entries of the compressor's hash table
constexpr uint32_t INPUT_MARGIN = 15;
constexpr uint32_t MIN_NON_LITERAL_BLOCK = 1 + 1 + INPUT_MARGIN;

// ---------------------------------------------------------------- CRC-32C
// Reflected CRC-32C (Castagnoli).  A register value is a polynomial over GF(2)
// with x^0 in bit 31; "n zero bytes more" is a multiplication by x^(8 n) mod P,
// so a block splits into segments: raw(0, A || B) = raw(0, A) x^(8 |B|) ^ raw(0, B),
// and the init value adds 0xFFFFFFFF x^(8 |M|).
constexpr uint32_t CRC_POLY = 0x82F63B78u;

SNAP_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}

// a b mod P
SNAP_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 n) mod P by square-and-multiply on the public length n
SNAP_HD uint32_t crc_xpow8(uint64_t n) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
    while (n) {
        if (n & 1) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
        n >>= 1;
    }
    return r;
}

// the register after p[0, n), from c (no init, no final xor)
SNAP_HD uint32_t crc_bytes(const uint32_t *tab, uint32_t c, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
    return c;
}

// lane's segment of a block of L bytes
SNAP_HD void crc_segment(size_t L, uint32_t lane, size_t *begin, size_t *end) {
    const size_t seg = (L + LANES - 1) / LANES;
    size_t b = size_t(lane) * seg;
    if (b > L) b = L;
    size_t e = b + seg;
    if (e > L) e = L;
    *begin = b;
    *end = e;
}

// lane's term of raw(0, block): its segment's register moved over the bytes behind it
SNAP_HD uint32_t crc_lane_term(const uint32_t *tab, const uint8_t *p, size_t L, uint32_t lane) {
    size_t b, e;
    crc_segment(L, lane, &b, &e);
    if (b == e) return 0;
    return crc_mul(crc_bytes(tab, 0, p + b, e - b), crc_xpow8(L - e));
}

// the masked CRC the framing format stores, from the XOR of the 64 terms
SNAP_HD uint32_t crc_finish(uint32_t terms, size_t L) {
    const uint32_t c = terms ^ crc_mul(0xFFFFFFFFu, crc_xpow8(L)) ^ 0xFFFFFFFFu;
    return ((c >> 15) | (c << 17)) + 0xA282EAD8u;
}

// ---------------------------------------------------------------- compress
SNAP_HD uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
SNAP_HD uint64_t load64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

template <class W>
SNAP_HD size_t put_varint(W &w, uint8_t *d, uint64_t v) {
    size_t i = 0;
    while (v >= 0x80) {
        w.put(d + i++, (uint8_t)(v | 0x80));
        v >>= 7;
    }
    w.put(d + i++, (uint8_t)v);
    return i;
}

template <class W>
SNAP_HD size_t emit_literal(W &w, uint8_t *d, const uint8_t *lit, size_t len) {
    const size_t n = len - 1;
    size_t i;
    if (n < 60) {
        w.put(d, (uint8_t)(n << 2));
        i = 1;
    } else if (n < 256) {
        w.put(d, 60 << 2);
        w.put(d + 1, (uint8_t)n);
        i = 2;
    } else {
        w.put(d, 61 << 2);
        w.put(d + 1, (uint8_t)n);
        w.put(d + 2, (uint8_t)(n >> 8));
        i = 3;
    }
    w.copy(d + i, lit, len);
    return i + len;
}

template <class W>
SNAP_HD size_t emit_copy(W &w, uint8_t *d, size_t offset, size_t len) {
    size_t i = 0;
    while (len >= 68) {  // length-64 copy-2
        w.put(d + i, (63 << 2) | 2);
        w.put(d + i + 1, (uint8_t)offset);
        w.put(d + i + 2, (uint8_t)(offset >> 8));
        i += 3;
        len -= 64;
    }
    if (len > 64) {  // length-60 copy-2, leaving 5..8 for a short copy
        w.put(d + i, (59 << 2) | 2);
        w.put(d + i + 1, (uint8_t)offset);
        w.put(d + i + 2, (uint8_t)(offset >> 8));
        i += 3;
        len -= 60;
    }
    if (len >= 12 || offset >= 2048) {
        w.put(d + i, (uint8_t)(((len - 1) << 2) | 2));
        w.put(d + i + 1, (uint8_t)offset);
        w.put(d + i + 2, (uint8_t)(offset >> 8));
        return i + 3;
    }
    w.put(d + i, (uint8_t)(((offset >> 8) << 5) | ((len - 4) << 2) | 1));
    w.put(d + i + 1, (uint8_t)offset);
    return i + 2;
}

// One block (MIN_NON_LITERAL_BLOCK <= n <= 64 KiB) without the varint header;
// `table` holds TABLE_MAX uint16 entries (LDS on the device).  dst is never read.
template <class W>
SNAP_HD size_t encode_block(W &w, uint8_t *dst, const uint8_t *src, size_t n, uint16_t *table) {
    uint32_t shift = 24;
    size_t tsize = 256;
    while (tsize < TABLE_MAX && tsize < n) {
        --shift;
        tsize <<= 1;
    }
    w.zero16(table, tsize);
    w.sync();
#define SNAP_HASH(u) ((size_t)(((uint32_t)(u) * 0x1E35A7BDu) >> shift))
    const size_t s_limit = n - INPUT_MARGIN;
    size_t next_emit = 0, d = 0, s = 1;
    size_t next_hash = SNAP_HASH(w.uni(load32(src + s)));
    for (;;) {
        size_t skip = 32, s_next = s, cand;
        for (;;) {
            s = s_next;
            const size_t step = skip >> 5;
            s_next = s + step;
            skip += step;
            if (s_next > s_limit) goto remainder;
            cand = w.uni((uint32_t)table[next_hash]);
            table[next_hash] = (uint16_t)s;
            next_hash = SNAP_HASH(w.uni(load32(src + s_next)));
            if (w.uni(load32(src + s)) == w.uni(load32(src + cand))) break;
        }
        d += emit_literal(w, dst + d, src + next_emit, s - next_emit);
        for (;;) {
            const size_t base = s;
            s += 4;
            s += w.match(src, cand + 4, s, n);  // the maximal common length up to the block's end
            d += emit_copy(w, dst + d, base - cand, s - base);
            next_emit = s;
            if (s >= s_limit) goto remainder;
            const uint64_t x = (uint64_t)w.uni(load32(src + s - 1)) | ((uint64_t)w.uni(load32(src + s + 3)) << 32);
            table[SNAP_HASH((uint32_t)x)] = (uint16_t)(s - 1);
            const size_t ch = SNAP_HASH((uint32_t)(x >> 8));
            cand = w.uni((uint32_t)table[ch]);
            table[ch] = (uint16_t)s;
            if ((uint32_t)(x >> 8) != w.uni(load32(src + cand))) {
                next_hash = SNAP_HASH((uint32_t)(x >> 16));
                ++s;
                break;
            }
        }
    }
remainder:
#undef SNAP_HASH
    if (next_emit < n) d += emit_literal(w, dst + d, src + next_emit, n - next_emit);
    return d;
}

// Raw snappy of one block (1 <= n <= 64 KiB), varint header included: what a
// compressed chunk's body would be.  At most MAX_COMPRESS_BLOCK bytes.
template <class W>
SNAP_HD size_t compress_block(W &w, uint8_t *dst, const uint8_t *src, size_t n, uint16_t *table) {
    size_t d = put_varint(w, dst, n);
    if (n < MIN_NON_LITERAL_BLOCK) return d + emit_literal(w, dst + d, src, n);
    return d + encode_block(w, dst + d, src, n, table);
}

// ---------------------------------------------------------------- decompress
SNAP_HD bool get_varint(const uint8_t *p, size_t n, uint64_t *v, size_t *used) {
    uint64_t r = 0;
    for (size_t i = 0; i < n && i < 10; ++i) {
        r |= (uint64_t)(p[i] & 0x7F) << (7 * i);
        if (!(p[i] & 0x80)) {
            *v = r;
            *used = i + 1;
            return true;
        }
    }
    return false;
}

// Raw snappy block decode of src[0, n) into stage[0, cap), cap <= MAX_BLOCK
// (LDS on the device); false on corrupt input.  Every read of src is below n,
// every write of stage below the block's own length, every iteration takes at
// least one byte of src: whatever the bytes are, it ends.
template <class W>
SNAP_HD bool decode_block(W &w, const uint8_t *src, size_t n, uint8_t *stage, size_t cap, size_t *out_len) {
    uint64_t dlen;
    size_t used;
    if (!get_varint(src, n, &dlen, &used) || dlen > cap) return false;
    size_t s = used, d = 0;
    while (s < n) {
        const uint32_t tag = w.uni((uint32_t)src[s]);
        size_t len, off;
        switch (tag & 3) {
            case 0: {  // literal
                size_t x = tag >> 2;
                if (x < 60) {
                    s += 1;
                } else {
                    const size_t nb = x - 59;  // 1..4 length bytes
                    if (s + 1 + nb > n) return false;
                    x = 0;
                    for (size_t b = 0; b < nb; ++b) x |= (size_t)w.uni((uint32_t)src[s + 1 + b]) << (8 * b);
                    s += 1 + nb;
                }
                len = x + 1;
                if (len > n - s || len > dlen - d) return false;
                w.copy(stage + d, src + s, len);
                w.sync();
                s += len;
                d += len;
                continue;
            }
            case 1:
                if (s + 2 > n) return false;
                len = 4 + ((tag >> 2) & 7);
                off = ((size_t)(tag >> 5) << 8) | w.uni((uint32_t)src[s + 1]);
                s += 2;
                break;
            case 2:
                if (s + 3 > n) return false;
                len = 1 + (tag >> 2);
                off = (size_t)w.uni((uint32_t)src[s + 1]) | ((size_t)w.uni((uint32_t)src[s + 2]) << 8);
                s += 3;
                break;
            default:
                if (s + 5 > n) return false;
                len = 1 + (tag >> 2);
                off = (size_t)w.uni((uint32_t)src[s + 1]) | ((size_t)w.uni((uint32_t)src[s + 2]) << 8) |
                      ((size_t)w.uni((uint32_t)src[s + 3]) << 16) | ((size_t)w.uni((uint32_t)src[s + 4]) << 24);
                s += 5;
                break;
        }
        if (off == 0 || off > d || len > dlen - d) return false;
        w.rep(stage, d, off, len);  // len <= 64
        w.sync();
        d += len;
    }
    if (d != dlen) return false;
    *out_len = d;
    return true;
}

// ---------------------------------------------------------------- tables (device scratch)
// Laid out by snap_plan.hpp, read and written by snap_kernels.hip.
struct CObj {  // compress: one object
    uint64_t in_off, n, out_off;
    uint32_t blk0, nblk;  // its blocks are blk0 .. blk0 + nblk - 1
};
static_assert(sizeof(CObj) == 32, "table layout");
struct CBlk {  // compress: one 64 KiB block
    uint32_t obj, idx;
};
struct CMeta {  // compress: what the block kernel and the frame kernel leave for the gather
    uint32_t clen, crc;
    uint64_t off;  // the chunk's offset in its stream; bit 63: stored raw
};
constexpr uint64_t CMETA_RAW = uint64_t(1) << 63;

struct UObj {  // decompress: one stream
    uint64_t in_off, in_len, out_off, out_cap;
    uint32_t slot0, nslots, pad0, pad1;
};
static_assert(sizeof(UObj) == 48, "table layout");
enum : uint32_t { CHUNK_NONE = 0, CHUNK_RAW = 1, CHUNK_COMPRESSED = 2 };
struct UDesc {  // decompress: one data chunk, as the walk found it
    uint64_t src;      // its data bytes, from d_in
    uint64_t out_pos;  // where its block starts in the object's output
    uint32_t dl, ulen, want, kind;
};
static_assert(sizeof(UDesc) == 32, "table layout");
struct UState {  // decompress: one stream after the walk
    uint32_t status, pad;
    uint64_t need;
};

// status codes of carbonado_hip.h the kernels write
constexpr uint32_t ST_OK = 0, ST_TOO_SMALL = 2, ST_UNSUPPORTED = 11, ST_SNAP = 16;

// ---------------------------------------------------------------- one thread as a wave
// The policy of the host check: the collective steps split as the kernel's 64
// lanes split them, run one lane after the other.
struct OneThread {
    void copy(uint8_t *dst, const uint8_t *src, size_t n) {
        for (uint32_t lane = 0; lane < LANES; ++lane)
            for (size_t i = lane; i < n; i += LANES) dst[i] = src[i];
    }
    size_t match(const uint8_t *src, size_t a, size_t b, size_t n) {
        for (size_t base = 0;; base += 8 * LANES) {
            uint64_t stop = 0;
            uint32_t cnt[LANES];
            for (uint32_t lane = 0; lane < LANES; ++lane) {
                const size_t at = base + 8 * lane;
                uint32_t c = 0;
                while (c < 8 && b + at + c < n && src[a + at + c] == src[b + at + c]) ++c;
                cnt[lane] = c;
                if (c < 8) stop |= uint64_t(1) << lane;
            }
            if (stop) {
                const uint32_t first = (uint32_t)__builtin_ctzll(stop);
                return base + 8 * first + cnt[first];
            }
        }
    }
    void zero16(uint16_t *t, size_t n) {
        for (size_t i = 0; i < n; ++i) t[i] = 0;
    }
    void put(uint8_t *p, uint8_t v) { *p = v; }
    void rep(uint8_t *stage, size_t d, size_t off, size_t c) {
        uint8_t v[LANES];
        for (uint32_t lane = 0; lane < c; ++lane) v[lane] = stage[d - off + lane % off];
        for (uint32_t lane = 0; lane < c; ++lane) stage[d + lane] = v[lane];
    }
    void sync() {}
    uint32_t uni(uint32_t x) { return x; }
};

}  // namespace snap
}  // namespace chip
