// fread_block.hpp — what a frame read does once a work item knows its request:
// the block decode of one (request, frame) by a 64-lane workgroup and the
// finish of one request by a 256-lane workgroup.  Device code (a workgroup
// barrier, LDS, readfirstlane) for KF (fread_kernels.hip), whose kernels take
// the work item from the uploaded tables, and KG (gread_kernels.hip), whose
// kernels build it from the request; fread_device.hpp stays the part the host
// check compiles.
#pragma once

#include "fread_device.hpp"
#include "snap_wave.hpp"

namespace chip {
namespace fread {

// rows + sg.src: the frame's chunk header in the staging rows; stage: 64 KiB of
// LDS; tab: 256 words of LDS.  The header against the index, snap::decode_block
// into LDS, snap::wave_crc, lane_store of the wanted bytes.  Returns the
// frame's verdict (true: its wanted bytes are stored); every lane of the
// workgroup calls it.
__device__ inline bool frame_block(const Seg &sg, const uint8_t *rows, uint8_t *content, uint8_t *stage, uint32_t *tab,
                                   uint32_t lane) {
    const uint8_t *h = rows + sg.src;
    bool ok = sg.clen >= 4;  // else the index leaves no room for a chunk here: nothing of the row is this frame's
    uint32_t ty = 0, want = 0;
    if (ok) {
        ty = h[0];
        const uint32_t clen = uint32_t(h[1]) | uint32_t(h[2]) << 8 | uint32_t(h[3]) << 16;
        want = snap::load32(h + 4);
        ok = ty <= 1 && clen == sg.clen;
    }
    ty = __builtin_amdgcn_readfirstlane(ty);
    ok = __builtin_amdgcn_readfirstlane(ok ? 1u : 0u) != 0;
    const uint32_t dl = sg.clen - 4;
    const uint8_t *from = stage;
    if (ok && ty == 1) {
        ok = dl == sg.ulen;
        from = h + 8;
    } else if (ok) {
        snap::Wave w{lane};
        size_t got = 0;
        ok = snap::decode_block(w, h + 8, dl, stage, sg.ulen, &got) && got == sg.ulen;
    }
    snap::crc_table_fill(tab, lane);
    __syncthreads();
    if (ok) ok = snap::wave_crc(tab, from, sg.ulen, lane) == want;
    if (ok) lane_store(content + sg.dst, from + sg.lo, sg.hi - sg.lo, lane);
    return ok;
}

// One request behind its block decodes, by every lane of a 256-lane workgroup.
// kill: a status decided before any work (0: none); n bytes at content; bad:
// its nbad verdict words, looked at only where its status word is still 0 (then
// every one was written); status, used, vouch: the call's result words, r its
// index in them.  An empty request that was not killed is served; a failed one
// keeps no byte.
__device__ inline void finish_request(uint32_t kill, uint64_t n, const uint32_t *bad, uint32_t nbad, uint8_t *content,
                                      uint32_t *status, uint32_t *used, uint32_t *vouch, uint32_t r, uint32_t tid) {
    __shared__ uint32_t any;
    if (!kill && n == 0) {  // nothing was asked of the stream: an empty request is served
        if (tid == 0) status[r] = 0;
        return;
    }
    uint32_t st = kill ? kill : status[r];
    if (tid == 0) any = 0;
    __syncthreads();
    if (st == 0)
        for (uint32_t k = tid; k < nbad; k += 256)
            if (bad[k]) any = 1;
    __syncthreads();
    if (st == 0 && any) st = ST_SNAP;
    if (st == 0) return;
    lane_zero(content, n, tid, 256);  // no byte of a failed request stays
    if (tid == 0) {
        status[r] = st;
        if (kill) {
            used[r] = 0;
            vouch[r] = 0;
        }
    }
}

}  // namespace fread
}  // namespace chip
