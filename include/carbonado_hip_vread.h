/*
 * carbonado_hip_vread.h — vouched ranged reads of libcarbonado_hip.so: the
 * ranged reads of carbonado_hip_read.h with every rebuilt chunk hashed against
 * the CV the stream's own tree stores for it, and a verdict per request that
 * says whether a hash vouches for each byte handed out.  Same library, same
 * conventions and status codes (chip_status) as carbonado_hip.h,
 * carbonado_hip_ext.h, carbonado_hip_audit.h, carbonado_hip_repair.h and
 * carbonado_hip_read.h, which stay frozen at their versions; every name here is
 * prefixed chipv_ and versioned by CHIPV_ABI_VERSION.
 *
 * Terms are those of carbonado_hip_read.h: stream, object, request, content,
 * segment (columns [c0, c1) of primary p), window [w0, w1), slice (segment, i),
 * authentic, and the selection rule "first four authentic shares ascending"
 * with its coefficients.  The layout call is chipd_read_layout of that header,
 * unchanged: its offsets, lengths and segment count serve this call.
 *
 * The verdict of a segment's own slice (g, p) is split in two:
 *   PATH(g)    every parent the slice selects, re-hashed from its stored bytes,
 *              equals the CV stored in its own parent (the root: d_hash);
 *   CHUNKS(g)  every chunk of the slice hashes to the CV stored in its nearest
 *              parent, and the stream's header equals its content length.
 * The slice is authentic exactly when both hold, as in carbonado_hip_read.h.
 *
 * Every segment gets one class:
 *   DIRECT        own slice authentic: the bytes are copied.
 *   FAILED        own slice not authentic and fewer than 4 of the other 7
 *                 slices authentic: no bytes.
 *   otherwise the segment is rebuilt as chipd_read_ranges_dev rebuilds it (same
 *   selected shares, same coefficients), and
 *   VOUCHED       PATH(g) holds and every chunk c of the window passes the chunk
 *                 check below: the rebuilt bytes are handed out.
 *   CONTRADICTED  PATH(g) holds and some window chunk fails the chunk check:
 *                 no bytes.  The stream's encoding contradicts its own tree.
 *   UNVOUCHED     PATH(g) does not hold: the stored CVs are not chained to the
 *                 root, so nothing can be compared.  The rebuilt bytes are
 *                 handed out with the guarantee of carbonado_hip_read.h.
 * The chunk check: chunk c of primary p is rebuilt in full, all 1024 columns
 * [1024 c, 1024 (c + 1)) from the four selected shares at the same columns
 * (the whole chunk, not only the requested bytes), hashed as BLAKE3 chunk
 * number p spc + c of the stream, and compared with the 32-byte CV stored for
 * that chunk in its nearest parent in the stream.  With PATH(g) that CV is
 * chained to the root, so equal means the rebuilt bytes are exactly as
 * authenticated as copied ones.  Every rebuilt segment with PATH is checked
 * whatever its request's other segments do: the classes of a call are a
 * function of the streams and the requests alone.
 *
 * Per-request results (device uint32 arrays, all three set for every request):
 * d_vouch[r] = the OR over its segments of CHIPV_VOUCHED (1), CHIPV_UNVOUCHED
 * (2), CHIPV_CONTRADICTED (4); DIRECT and FAILED segments add nothing.  0 for
 * an empty request and for one refused on the host (chunk_len or padding that
 * does not fit).
 * d_status[r] = CHIP_ERR_BAO_HASH_MISMATCH (5) if any segment is CONTRADICTED;
 * else CHIP_ERR_ZFEC (7) if any segment is FAILED, if the stream's chunk_len or
 * padding does not fit (as in carbonado_hip_read.h), or if flags has
 * CHIPV_STRICT and any segment is UNVOUCHED; else 0.
 * d_used[r] as in carbonado_hip_read.h: 0 for a failed request (any status but
 * 0), else the share bits.
 * Content is all or nothing per request, as there: the exact bytes for status
 * 0, zeros otherwise, no other byte of d_content touched, nothing past
 * scratch_len in d_scratch, and d_streams is never written.
 *
 * What this adds up to.
 *  - With status 0 and !(d_vouch[r] & CHIPV_UNVOUCHED), every byte handed out
 *    is hashed against the root.
 *  - With CHIPV_STRICT, status 0 alone says so.
 *  - With flags == 0, a request whose status here is 0 or 7 has the status,
 *    used word and content chipd_read_ranges_dev gives it; status 5 appears
 *    only where that call gives 0.
 *
 * Host arrays, the stream and the graph restriction are as in
 * carbonado_hip_read.h.  d_scratch belongs to the call until its work is done.
 *
 * Work per call: one table upload (the table of chipd_read_ranges_dev,
 * nothing added), one memset and at most 8 kernel launches whatever nreq, the
 * sizes, the ranges and the damage: KA's parent check of the primary slices
 * (the path word), KA's chunk check of them (the chunk word), the same two
 * checks of the fallback slices, gated on "either word set", the class per
 * segment, the vouch kernel (one quad of lanes per window chunk, gated: a quad
 * whose segment is not rebuilt under an intact path returns before it loads a
 * byte of a stream, so an intact call pays the launch and no hashing), the
 * verdict per request, the read.  Exactly 8 when the call has a segment; 1
 * (the verdict) when every request is empty or refused.  No synchronisation:
 * the call returns with everything enqueued on `stream`.
 *
 * Decided on the host before anything is enqueued, in this order:
 * CHIP_ERR_INVALID_ARG for a NULL array or buffer with nreq > 0 (d_vouch among
 * them; d_content only where some request has content), then for a bit of
 * flags other than CHIPV_STRICT, then everything carbonado_hip_read.h lists
 * from nreq >= 2^31 on, in its order, with chipv_read_scratch_len in the place
 * of chipd_read_scratch_len: the remaining CHIP_ERR_INVALID_ARG cases,
 * CHIP_ERR_BAO_TRUNCATED, CHIP_ERR_HASH_DECODE, CHIP_ERR_NO_DEVICE.
 * nreq == 0 is CHIP_OK and touches nothing, whatever the flags.
 */
#ifndef CARBONADO_HIP_VREAD_H
#define CARBONADO_HIP_VREAD_H

#include "carbonado_hip_read.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPV_API __attribute__((visibility("default")))
#else
#define CHIPV_API
#endif

#define CHIPV_ABI_VERSION 1

/* bits of d_vouch[r] */
#define CHIPV_VOUCHED 1u
#define CHIPV_UNVOUCHED 2u
#define CHIPV_CONTRADICTED 4u

/* flags: a request with an UNVOUCHED segment fails with CHIP_ERR_ZFEC */
#define CHIPV_STRICT 1u

CHIPV_API int chipv_abi_version(void);

/* Bytes of device scratch a call of nreq requests in nseg segments
 * (chipd_read_layout) needs: at least chipd_read_scratch_len(nreq, nseg), a
 * multiple of 16, growing with either.  Host only. */
CHIPV_API uint64_t chipv_read_scratch_len(uint64_t nreq, uint64_t nseg);

/* The content of every request, copied, or rebuilt and vouched for as above.
 * The arguments of chipd_read_ranges_dev, with d_vouch behind d_used and flags
 * in front of d_scratch.  d_status, d_used, d_vouch and the content are valid
 * once the work enqueued on `stream` is done. */
CHIPV_API int chipv_read_ranges_dev(const uint8_t *d_streams, const uint64_t *in_off, const uint64_t *in_len,
                                    const uint8_t *d_hash, const uint32_t *padding, const uint32_t *chunk_len,
                                    uint64_t nstreams, const uint32_t *req_stream, const uint64_t *start,
                                    const uint64_t *len, uint64_t nreq, uint8_t *d_content, const uint64_t *content_off,
                                    uint64_t *content_len, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch,
                                    uint32_t flags, void *d_scratch, uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_VREAD_H */
