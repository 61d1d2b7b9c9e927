// fread_device.hpp — what KF (fread_kernels.hip) computes, as __host__
// __device__ code: the parse of one
// chunk header of a frame stream, the serial walk over the headers, the
// verdict of one link of a frame index, and the store of a sub-range of a
// decoded block.  One text for the kernels and for the stand-alone check
// (tests/fread_device_check.cpp), as snap_device.hpp is for KZ.
//
// A frame stream is CANONICAL when it is empty, or the 10-byte stream
// identifier followed by data chunks only (type 0x00 compressed, 0x01 raw),
// every chunk but the last holding 65536 uncompressed bytes and the last 1 to
// 65536, ending exactly at the stream's end.  Frame lengths are public: they
// drive addresses and branches here, as they do in KZ.
#pragma once

#include "cread_device.hpp"
#include "snap_device.hpp"

namespace chip {
namespace fread {

constexpr uint32_t FRAME = snap::MAX_BLOCK;  // uncompressed bytes of every frame but the last
constexpr uint32_t ID_LEN = 10;              // the stream identifier
constexpr uint32_t HDR_READ = 12;            // header (4), CRC (4) and the up to 3 varint bytes of a length <= 65536
constexpr uint32_t ROW = 16;                 // a header's staging row
constexpr uint32_t LANES = snap::LANES;
constexpr uint32_t ST_OK = 0, ST_TOO_SMALL = 2, ST_HASH = 5, ST_ZFEC = 7, ST_UNSUPPORTED = 11, ST_SNAP = 16;

// ---- one chunk header ---------------------------------------------------------------
struct Hdr {
    uint32_t verdict;  // ST_OK: a data chunk of 1..65536 bytes; ST_UNSUPPORTED: valid, not canonical; ST_SNAP
    uint32_t clen;     // the header's 24-bit length
    uint32_t ulen;     // uncompressed bytes (ST_OK only)
};

// b: frame-stream bytes [pos, min(pos + 12, L)) (whatever lies behind them in b is not looked at)
SNAP_HD Hdr parse_header(const uint8_t *b, uint64_t pos, uint64_t L) {
    Hdr h{ST_SNAP, 0, 0};
    if (pos >= L || L - pos < 4) return h;
    const uint32_t ty = b[0];
    h.clen = uint32_t(b[1]) | uint32_t(b[2]) << 8 | uint32_t(b[3]) << 16;
    if (h.clen > L - pos - 4) return h;  // ends behind the stream
    if (ty >= 0x80) {  // a skippable chunk, padding or a repeated identifier
        h.verdict = ST_UNSUPPORTED;
        return h;
    }
    if (ty > 1 || h.clen < 4) return h;  // reserved unskippable, or no room for the CRC
    const uint64_t avail = L - pos < HDR_READ ? L - pos : HDR_READ;  // >= 8 here
    const uint32_t dl = h.clen - 4;
    uint64_t ulen = dl;
    if (ty == 0) {
        size_t used;
        const uint64_t nv = avail - 8 < dl ? avail - 8 : dl;
        if (!snap::get_varint(b + 8, size_t(nv), &ulen, &used)) return h;
    }
    if (ulen > FRAME) return h;
    h.ulen = uint32_t(ulen);
    h.verdict = ulen ? ST_OK : ST_UNSUPPORTED;  // an empty block decodes, no encoder here writes one
    return h;
}

SNAP_HD bool ident_ok(const uint8_t *b) {
    const uint8_t id[ID_LEN] = {0xFF, 0x06, 0x00, 0x00, 's', 'N', 'a', 'P', 'p', 'Y'};
    bool ok = true;
    for (uint32_t i = 0; i < ID_LEN; ++i) ok = ok && b[i] == id[i];
    return ok;
}

// ---- the walk ---------------------------------------------------------------------
struct WalkOut {
    uint32_t status;   // 0, ST_TOO_SMALL, ST_UNSUPPORTED or ST_SNAP
    uint32_t nframes;  // data chunks found (counted past the capacity)
    uint64_t plain;    // their uncompressed bytes
    uint64_t bad_pos;  // where the walk stopped, status 11 or 16
};
static_assert(sizeof(WalkOut) == 24, "record layout");

// fetch(pos, n, b): frame-stream bytes [pos, pos + n), n <= 12, into b.  off:
// the stream's cap entries.  Every hop advances by at least 8 bytes (the 4-byte
// header and the CRC a data chunk must hold) and ends at
// L, at a header that is not a canonical data chunk, or never past cap entries
// written.  A stream that stops early leaves the position of the header it
// stopped at behind the entries found, where there is room.
template <class F>
SNAP_HD WalkOut walk(F &fetch, uint64_t L, uint64_t *off, uint32_t cap) {
    WalkOut o{ST_OK, 0, 0, 0};
    if (L == 0) {
        if (cap >= 1) off[0] = 0;
        else o.status = ST_TOO_SMALL;
        return o;
    }
    uint8_t b[HDR_READ];
    uint64_t pos = ID_LEN;
    if (L < ID_LEN) {
        o.status = ST_SNAP;
    } else {
        fetch(uint64_t(0), ID_LEN, b);
        if (!ident_ok(b)) o.status = ST_SNAP;
        else if (L == ID_LEN) o.status = ST_UNSUPPORTED;  // an identifier and no chunk
    }
    while (o.status == ST_OK && pos < L) {
        const uint32_t n = uint32_t(L - pos < HDR_READ ? L - pos : HDR_READ);
        fetch(pos, n, b);
        const Hdr h = parse_header(b, pos, L);
        uint32_t v = h.verdict;
        if (v == ST_OK && pos + 4 + h.clen != L && h.ulen != FRAME) v = ST_UNSUPPORTED;  // a short inner block
        if (v != ST_OK) {
            o.status = v;
            o.bad_pos = pos;
            break;
        }
        if (o.nframes < cap) off[o.nframes] = pos;
        ++o.nframes;
        o.plain += h.ulen;
        pos += 4 + uint64_t(h.clen);
    }
    if (o.status == ST_OK) {
        if (o.nframes < cap) off[o.nframes] = L;
        else o.status = ST_TOO_SMALL;
    } else if (o.nframes < cap) {
        off[o.nframes] = o.bad_pos;
    }
    return o;
}

// ---- one link of an index ------------------------------------------------------------
// b: the staged bytes of the header at `off`; next: the entry behind it; last:
// it is the index's last frame.  *ulen is set for ST_OK.
SNAP_HD uint32_t link_verdict(const uint8_t *b, uint64_t off, uint64_t next, bool last, uint64_t L, uint32_t *ulen) {
    const Hdr h = parse_header(b, off, L);
    if (h.verdict == ST_SNAP) return ST_SNAP;
    if (off + 4 + uint64_t(h.clen) != next || (last && next != L)) return ST_SNAP;
    if (h.verdict != ST_OK) return h.verdict;
    if (!last && h.ulen != FRAME) return ST_UNSUPPORTED;
    *ulen = h.ulen;
    return ST_OK;
}
// the verdicts of a stream's links and header reads as one status: a read that
// could not be served first (5 before 7), then 16, then 11
SNAP_HD uint32_t chain_status(bool hash, bool zfec, bool snap_bad, bool unsupported) {
    return hash ? ST_HASH : zfec ? ST_ZFEC : snap_bad ? ST_SNAP : unsupported ? ST_UNSUPPORTED : ST_OK;
}

// ---- the read's work items ----------------------------------------------------------
struct Seg {  // one (request, frame)
    uint64_t src;   // of the frame's header in the staging region
    uint64_t dst;   // of the first byte it stores, in d_content
    uint32_t req;
    uint32_t clen;  // what the header must say: off[f + 1] - off[f] - 4; below 4: the index leaves no room for a chunk
    uint32_t ulen;  // the frame's uncompressed bytes by the index
    uint32_t lo, hi;  // the bytes of the frame that the request wants
    uint32_t pad_;
};
static_assert(sizeof(Seg) == 40, "record layout");

struct Req {
    uint64_t dst, n;  // the content range
    uint32_t seg0, nseg;
    uint32_t kill;  // the stream's index_status: zeros and this status, no work
    uint32_t pad_;
};
static_assert(sizeof(Req) == 32, "record layout");

// lane's share of n bytes from src to dst, both at any byte address: bytes up to
// dst's next 16-B boundary, 16-B stores from there (16-B loads where src has
// the same residue, else four unaligned words), bytes at the end
SNAP_HD void lane_store(uint8_t *dst, const uint8_t *src, size_t n, uint32_t lane) {
    size_t head = size_t(0 - reinterpret_cast<uintptr_t>(dst)) & 15;
    if (head > n) head = n;
    const size_t body = (n - head) / 16;
    for (size_t i = lane; i < head; i += LANES) dst[i] = src[i];
    const bool same = ((reinterpret_cast<uintptr_t>(src + head)) & 15) == 0;
    for (size_t u = lane; u < body; u += LANES) {
        const uint8_t *s = src + head + 16 * u;
        uint32_t w[4];
        if (same) {
            __builtin_memcpy(w, __builtin_assume_aligned(s, 16), 16);
        } else {
            for (int c = 0; c < 4; ++c) w[c] = snap::load32(s + 4 * c);
        }
        __builtin_memcpy(__builtin_assume_aligned(dst + head + 16 * u, 16), w, 16);
    }
    for (size_t i = head + 16 * body + lane; i < n; i += LANES) dst[i] = src[i];
}

// lane's share of n zero bytes at any byte address
SNAP_HD void lane_zero(uint8_t *dst, uint64_t n, uint32_t lane, uint32_t lanes) {
    uint64_t head = uint64_t(0 - reinterpret_cast<uintptr_t>(dst)) & 15;
    if (head > n) head = n;
    const uint64_t body = (n - head) / 16;
    const uint32_t z[4] = {0, 0, 0, 0};
    for (uint64_t i = lane; i < head; i += lanes) dst[i] = 0;
    for (uint64_t u = lane; u < body; u += lanes) __builtin_memcpy(__builtin_assume_aligned(dst + head + 16 * u, 16), z, 16);
    for (uint64_t i = head + 16 * body + lane; i < n; i += lanes) dst[i] = 0;
}

// ---- tables of the index calls ---------------------------------------------------------
struct WStream {  // the walk: one stream
    uint64_t src;  // of the stream in d_streams
    uint64_t L;    // bytes of its frame stream
    uint64_t ent0; // its first entry in the call's offsets
    uint32_t N;    // chunks of the bao stream
    uint32_t cap;  // entries it may write
    uint32_t shift;  // object byte of frame-stream byte 0: 0, or 97 behind an envelope's header
    uint32_t skip;   // a status decided on the host: no work
    uint32_t key;    // its CtrKey, where shift != 0
    uint32_t pad_;
};
static_assert(sizeof(WStream) == 48, "record layout");

struct VStream {  // the chain check: one stream
    uint64_t L;
    uint64_t ent0;   // its first entry in the uploaded offsets; its first staging row and read (the identifier's)
    uint32_t nframes;
    uint32_t skip;
};
static_assert(sizeof(VStream) == 24, "record layout");

// The chain check of one stream by one lane of `lanes` (frames f = lane, lane +
// lanes, ...): what this lane saw, as bits: 1 a read with status 5, 2 one with
// 7, 4 a link that is wrong, 8 one that is not canonical; the vouch bits ORed
// into *vouch, the last frame's length into *last_ulen by the lane that has it.
SNAP_HD uint32_t chain_lane(const VStream &v, const uint64_t *off, const uint8_t *rows, const uint32_t *rstat,
                            const uint32_t *rvouch, uint32_t lane, uint32_t lanes, uint32_t *vouch,
                            uint32_t *last_ulen) {
    uint32_t bits = 0;
    if (lane == 0) {  // the identifier, and the shapes without a frame
        if (v.L == 0) {
            if (v.nframes != 0 || off[0] != 0) bits |= 4;
        } else {
            *vouch |= rvouch[0];
            if (rstat[0]) bits |= rstat[0] == ST_HASH ? 1 : 2;
            else if (v.L < ID_LEN || !ident_ok(rows) || off[0] != ID_LEN) bits |= 4;
            else if (v.nframes == 0) bits |= v.L == ID_LEN ? 8 : 4;  // an identifier alone is valid, not canonical
        }
    }
    for (uint64_t f = lane; v.L && f < v.nframes; f += lanes) {
        *vouch |= rvouch[1 + f];
        if (rstat[1 + f]) {
            bits |= rstat[1 + f] == ST_HASH ? 1 : 2;
            continue;
        }
        uint32_t ulen = 0;
        const bool last = f + 1 == v.nframes;
        const uint32_t s = link_verdict(rows + ROW * (1 + f), off[f], off[f + 1], last, v.L, &ulen);
        if (s == ST_SNAP) bits |= 4;
        else if (s == ST_UNSUPPORTED) bits |= 8;
        else if (last) *last_ulen = ulen;
    }
    return bits;
}

}  // namespace fread
}  // namespace chip
