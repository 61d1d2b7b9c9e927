// gread_block.hpp — the block decode of one (request, frame) work item by one
// 64-lane workgroup, device code for gread_kernels.hip.  It is the body of KF's
// fread_block_kernel (fread_kernels.hip) behind its table load and its gate,
// statement for statement: the header against the index, snap::decode_block
// into LDS, snap::wave_crc, fread::lane_store of the wanted bytes.  It stands
// here and not in fread_device.hpp because the older boundaries stay frozen,
// kernels included: moving the text out of fread_block_kernel would recompile
// that kernel, and its code is what the host-planned call is measured by.
#pragma once

#include "fread_device.hpp"
#include "snap_wave.hpp"

namespace chip {
namespace gread {

// rows + sg.src: the frame's chunk header in the staging rows; stage: 64 KiB of
// LDS; tab: 256 words of LDS.  Returns the frame's verdict (true: its wanted
// bytes are stored); every lane of the workgroup calls it.
__device__ inline bool frame_block(const fread::Seg &sg, const uint8_t *rows, uint8_t *content, uint8_t *stage,
                                   uint32_t *tab, uint32_t lane) {
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
    if (ok) fread::lane_store(content + sg.dst, from + sg.lo, sg.hi - sg.lo, lane);
    return ok;
}

}  // namespace gread
}  // namespace chip
