// fread_kernels.hip — KF: the frame index of resident level-14 / level-15
// streams and the block decode of a ranged read.  The header parse, the walk,
// the chain check and the sub-range store are in fread_device.hpp (shared with
// the host check); the decode of one frame and the finish of one request are in
// fread_block.hpp (shared with KG, whose kernels build the work item from the
// request); the block decoder and the CRC are KZ's (snap_device.hpp,
// snap_wave.hpp); the keystream of a hop is KC's (cread_device.hpp).  This file
// maps lanes and waves to streams and work items.
//
// No address and no branch here depends on a key, a round key, J0 or
// keystream: the walk's keystream stays in registers until it is XORed over the
// 12 fetched bytes, which are indexed by a loop counter.  What the XOR gives is
// plaintext of the object (chunk types and lengths) and does drive the walk.
// Every loop is bounded by a length from a table or a header that was checked
// against the stream's end, and no store leaves the entries, words or content
// range the table gives.
#include "fread_kernels.hpp"

#include "bao_device.hpp"
#include "fread_block.hpp"

namespace chip {
namespace {

using namespace fread;

// frame-stream bytes from the primary copy in the stream, decrypted where there
// is a key.  Object byte x of a Zfec|Bao stream is content byte x (the four
// primary shards are the first 4 chunk_len bytes of the content): chunk x / 1024
// at bao_device.hpp's chunk_stream_off.
struct Fetch {
    const uint8_t *stream;
    uint64_t N;
    uint32_t shift;
    const cread::CtrKey *k;
    __device__ void operator()(uint64_t pos, uint32_t n, uint8_t *b) const {
        const uint64_t x = shift + pos;
        uint64_t base = bao::chunk_stream_off(x / 1024, N);
        uint32_t in = uint32_t(x % 1024);
        for (uint32_t i = 0; i < HDR_READ; ++i) {
            uint8_t v = 0;
            if (i < n) {
                if (in == 1024) {  // the bytes go on in the next chunk
                    base = bao::chunk_stream_off((x + i) / 1024, N);
                    in = 0;
                }
                v = stream[base + in];
                ++in;
            }
            b[i] = v;
        }
        if (k) {
            cread::Item it{};
            it.pos = pos;
            uint32_t ka[4], kb[4], ks[4];
            cread::lane_eval(k, it, 0, 0, ka, kb);
            cread::ks_shift(ka, kb, uint32_t(pos & 15u), ks);
            for (uint32_t i = 0; i < HDR_READ; ++i)
                if (i < n) b[i] ^= uint8_t(ks[i >> 2] >> (8 * (i & 3)));
        }
    }
};

__global__ __launch_bounds__(64) void fread_walk_kernel(WalkLaunch L) {
    const uint32_t s = blockIdx.x * LANES + threadIdx.x;
    if (s >= L.count) return;
    const WStream w = L.streams[s];
    if (w.skip) {
        L.out[s] = WalkOut{w.skip, 0, 0, 0};
        return;
    }
    Fetch f{L.in + w.src, w.N, w.shift, w.shift ? L.km + w.key : nullptr};
    L.out[s] = walk(f, w.L, L.off + w.ent0, w.cap);
}

__device__ inline uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= uint32_t(__shfl_xor(int(v), d, LANES));
    return v;
}

__global__ __launch_bounds__(64) void fread_chain_kernel(ChainLaunch L) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const VStream v = L.streams[s];
    if (v.skip) {
        if (lane == 0) {
            L.status[s] = v.skip;
            L.plain[s] = 0;
            L.vouch[s] = 0;
        }
        return;
    }
    uint32_t vouch = 0, last_ulen = 0;
    uint32_t bits = chain_lane(v, L.off + v.ent0, L.rows + ROW * v.ent0, L.rstat + v.ent0, L.rvouch + v.ent0, lane,
                               LANES, &vouch, &last_ulen);
    bits = wave_or(bits);
    vouch = wave_or(vouch);
    last_ulen = wave_or(last_ulen);  // one lane has it, the others 0
    if (lane == 0) {
        const uint32_t st = chain_status(bits & 1, bits & 2, bits & 4, bits & 8);
        L.status[s] = st;
        L.plain[s] = st == ST_OK && v.nframes ? uint64_t(FRAME) * (v.nframes - 1) + last_ulen : 0;
        L.vouch[s] = vouch;
    }
}

__global__ __launch_bounds__(64) void fread_block_kernel(FrameLaunch L) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[FRAME];
    __shared__ uint32_t tab[256];
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const Seg sg = L.segs[g];
    // the read failed: the finish kernel zeroes the range.  bad[g] stays unwritten: fread_finish_kernel
    // looks at a request's bad words only where its status word is still 0, and then every one was written
    if (L.status[sg.req] != 0) return;
    const bool ok = frame_block(sg, L.rows, L.content, stage, tab, lane);
    if (lane == 0) L.bad[g] = ok ? 0u : 1u;
}

__global__ __launch_bounds__(256) void fread_finish_kernel(FrameLaunch L) {
    const uint32_t r = blockIdx.x;
    const Req q = L.reqs[r];
    finish_request(q.kill, q.n, L.bad + q.seg0, q.nseg, L.content + q.dst, L.status, L.used, L.vouch, r,
                   threadIdx.x);
}

}  // namespace

hipError_t fread_walk_launch(const WalkLaunch &L, hipStream_t stream) {
    if (L.count == 0) return hipSuccess;
    hipLaunchKernelGGL(fread_walk_kernel, dim3((L.count + LANES - 1) / LANES), dim3(LANES), 0, stream, L);
    return hipGetLastError();
}

hipError_t fread_chain_launch(const ChainLaunch &L, hipStream_t stream) {
    if (L.count == 0) return hipSuccess;
    hipLaunchKernelGGL(fread_chain_kernel, dim3(L.count), dim3(LANES), 0, stream, L);
    return hipGetLastError();
}

hipError_t fread_block_launch(const FrameLaunch &L, hipStream_t stream) {
    if (L.nseg == 0) return hipSuccess;
    hipLaunchKernelGGL(fread_block_kernel, dim3(L.nseg), dim3(LANES), 0, stream, L);
    return hipGetLastError();
}

hipError_t fread_finish_launch(const FrameLaunch &L, hipStream_t stream) {
    if (L.nreq == 0) return hipSuccess;
    hipLaunchKernelGGL(fread_finish_kernel, dim3(L.nreq), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace chip
