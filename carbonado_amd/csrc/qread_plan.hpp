// qread_plan.hpp — host side of the device-planned ranged reads
// (include/carbonado_hip_qread.h): the stream table and its one upload, the
// O(1) host work of a read call (argument checks, segment slots, grid bounds,
// scratch layout).  The requests themselves are planned on the device
// (qread_device.hpp, qread_kernels.hip); the host never sees them, so every grid
// of a call is a BOUND from (info, nreq, max_len), not a total.
// Pure host code without a HIP type in it (tests/qread_plan_check.cpp drives it
// under a sanitizer).
#pragma once

#include "../../include/carbonado_hip_qread.h"
#include "qread_device.hpp"
#include "vread_plan.hpp"

namespace chip {
namespace qread {

using read::up;

constexpr uint64_t SCAN_TILE = 1024;  // entries of a prefix array per workgroup of the scan kernels
constexpr uint32_t SCAN_ARRAYS = 4;   // parents, chunks, fallback parents, blocks

// ---- the stream table ------------------------------------------------------------
// [nstreams records | read::mask_table()], the masks on a 256-B boundary.
inline uint64_t table_masks_off(uint64_t nstreams) { return up(nstreams * sizeof(StreamRec), 256); }
inline uint64_t table_len(uint64_t nstreams) {
    if (nstreams >= (1ull << 32)) return 0;  // a request names its stream in 32 bits
    return table_masks_off(nstreams) + 256 * sizeof(read::MaskEntry);
}

// The checks read::plan_read makes per stream, in its order, and the table as
// uploaded.  Addresses are plain integers here.
inline int plan_table(uintptr_t d_streams, const uint64_t *in_off, const uint64_t *in_len, uintptr_t d_hash,
                      const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams, uintptr_t d_table,
                      uint64_t table_len_given, chipq_table_info *info, std::vector<uint8_t> *table) {
    if (!info) return CHIP_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    if (nstreams && (!d_streams || !in_off || !in_len || !padding || !chunk_len)) return CHIP_ERR_INVALID_ARG;
    if (!d_table || d_table % 16 || nstreams >= (1ull << 32)) return CHIP_ERR_INVALID_ARG;
    std::vector<uint64_t> n;
    bool truncated = false;
    const int st = audit::stream_lengths(d_streams, in_off, in_len, nstreams, &n, &truncated);
    if (st != CHIP_OK) return st;
    if (table_len_given < table_len(nstreams)) return CHIP_ERR_INVALID_ARG;
    if (truncated) return CHIP_ERR_BAO_TRUNCATED;
    if (!d_hash) return CHIP_ERR_HASH_DECODE;
    table->assign(table_len(nstreams), 0);
    StreamRec *recs = reinterpret_cast<StreamRec *>(table->data());
    info->nstreams = nstreams;
    for (uint64_t s = 0; s < nstreams; ++s) {
        StreamRec &q = recs[s];
        q.src = d_streams + in_off[s];
        q.n = n[s];
        q.N = audit::chunks(n[s]);
        q.hash = d_hash + 32 * s;
        const uint64_t C = repair::shard_len_of(n[s], chunk_len[s]);
        q.C = padding[s] > read::K * C ? 0 : (uint32_t)C;
        q.padding = padding[s];
        info->max_chunks = std::max<uint64_t>(info->max_chunks, q.N);
        if (q.C && (!info->min_shard || q.C < info->min_shard)) info->min_shard = q.C;
    }
    std::memcpy(table->data() + table_masks_off(nstreams), read::mask_table().data(), 256 * sizeof(read::MaskEntry));
    return CHIP_OK;
}

// ---- segment slots and grid bounds -------------------------------------------------
// A range of max_len bytes or fewer meets at most 1 + ceil((max_len - 1) / C)
// primaries of shard length C >= min_shard, and never more than K.
inline uint32_t slots_of(uint64_t min_shard, uint64_t max_len) {
    if (!min_shard) return 1;  // no stream fits: no request has a segment
    return (uint32_t)audit::umin(read::K, 1 + (max_len - 1 + min_shard - 1) / min_shard);
}

// Chunks a range of max_len bytes or fewer touches, over all its segments
// (segments end on chunk boundaries, so no chunk is counted twice).
inline uint64_t window_bound(uint64_t max_len) { return (max_len + 1022) / 1024 + 1; }

// Parents a slice of w >= 1 chunks selects of a tree of N chunks or fewer, at
// most: at level L the selected parents q lie in [f >> L, (l - 1) >> L] with
// l - f = w, which are at most ((w - 1) >> L) + 2, and the level has no more
// than np_L, which grows with N.
inline uint64_t slice_parents_bound(uint64_t N, uint64_t w) {
    uint64_t total = 0, cnt = N;
    for (int L = 1; cnt > 1; ++L) {
        total += audit::umin(cnt / 2, ((w - 1) >> L) + 2);
        cnt = (cnt + 1) / 2;
    }
    return total;
}

// Workgroups of the read kernel for one request: a segment of l bytes at any
// address has at most (l + 30) / 16 units (read::units_of), so at most
// (l + 30 + 4095) / 4096 blocks; over S segments of max_len bytes together the
// floors sum to no more than the floor of the sum.
inline uint64_t request_blocks_bound(uint64_t max_len, uint32_t S) {
    return (max_len + S * (2 * (read::UNIT - 1) + read::BLOCK - 1)) / read::BLOCK;
}

struct Geometry {
    uint32_t S = 0;
    uint64_t nslot = 0;  // S nreq: what the kernels take for the segment count
    // bounds of the work items of a call (the fallback chunk items are 7 x the chunk items on both sides)
    uint64_t parents = 0, chunks = 0, fb_parents = 0, blocks = 0;
    uint64_t scan_blocks = 0;  // workgroups per prefix array of the scan
    bool ok = false;           // every bound below 2^36 items and 2^31 workgroups or slots
    Geometry() {}
    Geometry(const chipq_table_info &info, uint64_t nreq, uint64_t max_len) {
        S = slots_of(info.min_shard, max_len);
        nslot = S * nreq;
        const uint64_t W = window_bound(max_len);
        const unsigned __int128 one = 1;
        // every slice of a request has W chunks or fewer, and its 7 shifted windows as many
        const unsigned __int128 par = one * nreq * S * slice_parents_bound(info.max_chunks, W);
        const unsigned __int128 chk = one * nreq * W, blk = one * nreq * request_blocks_bound(max_len, S);
        ok = nslot < (1ull << 31) && read::FALLBACKS * par < audit::MAX_ITEMS &&
             read::FALLBACKS * chk < audit::MAX_ITEMS && blk < (1ull << 31);
        if (!ok) return;
        parents = (uint64_t)par; chunks = (uint64_t)chk; blocks = (uint64_t)blk;
        fb_parents = read::FALLBACKS * parents;
        scan_blocks = (nslot + 1 + SCAN_TILE - 1) / SCAN_TILE;
    }
};

// ---- the scratch -----------------------------------------------------------------
// [slice requests | parents | chunks | fallback parents | blocks (the four
// prefix arrays) | block sums of the scan | requests | segments | 8 status
// words per slot | how each slot is served | path word | contradiction word
// per slot (vouched)], every region on a 256-B boundary.  The status, path and
// contradiction words are zeroed by the request kernel, slot by slot; `served`
// is written by the verdict kernels before it is read.
struct ScratchLayout {
    uint64_t slices = 0, parents = 0, chunks = 0, fpar = 0, blocks = 0, sums = 0, reqs = 0, segs = 0, rstat = 0,
             served = 0, path = 0, contra = 0, total = 0;
    uint64_t prefix_pitch = 0;  // bytes from one prefix array to the next
    ScratchLayout() {}
    ScratchLayout(const Geometry &g, uint64_t nreq, bool vouched) {
        prefix_pitch = up((g.nslot + 1) * 8, 256);
        parents = up(g.nslot * sizeof(audit::Req), 256);
        chunks = parents + prefix_pitch;
        fpar = chunks + prefix_pitch;
        blocks = fpar + prefix_pitch;
        sums = blocks + prefix_pitch;
        reqs = sums + up(SCAN_ARRAYS * g.scan_blocks * 8, 256);
        segs = reqs + up(nreq * sizeof(read::Req), 256);
        rstat = segs + up(g.nslot * sizeof(read::Seg), 256);
        served = rstat + up(read::M * g.nslot * 4, 256);
        path = served + up(g.nslot * sizeof(read::Served), 256);
        contra = vouched ? path + up(g.nslot * 4, 256) : path;
        total = vouched ? contra + up(g.nslot * 4, 256) : path;
    }
};

inline bool range_ok(uint64_t max_len) { return max_len != 0 && max_len <= read::MAX_RANGE; }

inline uint64_t scratch_len(const chipq_table_info *info, uint64_t nreq, uint64_t max_len, bool vouched) {
    if (!info || nreq >= (1ull << 31) || !range_ok(max_len)) return 0;
    const Geometry g(*info, nreq, max_len);
    return g.ok ? ScratchLayout(g, nreq, vouched).total : 0;
}

// The host checks of a read call, in the header's order; everything but the device.
inline int plan_call(uintptr_t d_table, const chipq_table_info *info, bool have_requests, uint64_t nreq,
                     uint64_t max_len, uintptr_t d_content, uint64_t content_stride, bool have_results, bool vouched,
                     uint32_t flags, uintptr_t d_scratch, uint64_t scratch_len_given, Geometry *g, ScratchLayout *lay) {
    if (nreq == 0) return CHIP_OK;
    if (!d_table || !info || !have_requests || !d_content || !have_results || !d_scratch) return CHIP_ERR_INVALID_ARG;
    if (nreq >= (1ull << 31) || !range_ok(max_len)) return CHIP_ERR_INVALID_ARG;
    if (content_stride % 16 || content_stride < up(max_len, 16) || content_stride > (~0ull - d_content) / nreq ||
        d_content % 16 || d_table % 16 || d_scratch % 16)
        return CHIP_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)CHIPV_STRICT) return CHIP_ERR_INVALID_ARG;
    *g = Geometry(*info, nreq, max_len);
    if (!g->ok) return CHIP_ERR_INVALID_ARG;
    *lay = ScratchLayout(*g, nreq, vouched);
    if (scratch_len_given < lay->total) return CHIP_ERR_INVALID_ARG;
    return CHIP_OK;
}

}  // namespace qread
}  // namespace chip
