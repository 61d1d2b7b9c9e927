/*
 * carbonado_hip_fread.h — plaintext ranged reads of level-14 (Snappy | Zfec |
 * Bao) and level-15 (Snappy | Ecies | Zfec | Bao) objects that stay in HBM, in
 * libcarbonado_hip.so: the vouched ranged reads of carbonado_hip_vread.h over
 * the compressed frames behind a range, the keystream of carbonado_hip_cread.h
 * taken off them at level 15, and one snappy block decode per frame.  Same
 * library, same conventions and status codes (chip_status) as carbonado_hip.h,
 * carbonado_hip_ext.h, carbonado_hip_audit.h, carbonado_hip_repair.h,
 * carbonado_hip_read.h, carbonado_hip_vread.h, carbonado_hip_ecies.h,
 * carbonado_hip_snap.h and carbonado_hip_cread.h, which stay frozen at their
 * versions; every name here is prefixed chipf_ and versioned by
 * CHIPF_ABI_VERSION.  Every older entry point keeps serving a level-14 or
 * level-15 stream as the level-12 stream of its frame stream or envelope,
 * exactly as before.  Formats served: 14 and 15 only.
 *
 * Terms.  The FRAME STREAM of stream s is its object at level 12:
 * L = 4 chunk_len[s] - padding[s] bytes at 14, and that minus 97 at 15 (0 where
 * negative).  It is the 10-byte stream identifier followed by one chunk per
 * 64 KiB block of the plaintext: a 4-byte header (type, 24-bit length), the
 * masked CRC-32C of the uncompressed block, and a body that decodes on its
 * own.  Every block but the last is full (carbonado_hip_snap.h), so plaintext
 * byte x lies in frame x / 65536.
 * A FRAME INDEX is host data: nframes[s] + 1 ascending uint64 offsets into the
 * frame stream; entry f is the first header byte of data chunk f, the last
 * entry is L.  An empty stream (L = 0) has nframes = 0 and the one entry 0.
 * A stream is CANONICAL when it is empty or consists of exactly the identifier
 * at [0, 10), then data chunks only, of type 0x00 or 0x01, every chunk but the
 * last with uncompressed length 65536, the last with 1..65536, ending exactly
 * at L.  FrameEncoder and this library write nothing else.  Valid streams that
 * are not canonical (skippable chunks, a repeated identifier, short inner
 * blocks, empty blocks, an identifier alone) get CHIP_ERR_UNSUPPORTED_FORMAT
 * (11) from the index calls; they go through chips_decode_ragged_dev.
 * plain_len[s] = 65536 (nframes - 1) + ulen(last).
 * Index arrays are laid out the way the ragged calls lay out rows: idx_off[s]
 * is an entry offset into one frame_off array, idx_cap[s] the number of
 * entries available to stream s.
 *
 * Host arrays are read at call time (so the calls cannot be captured into a
 * graph); d_* pointers are device memory; `stream` is a hipStream_t or NULL;
 * d_scratch belongs to the call until its work is done.  The number of kernel
 * launches does not depend on the batch.  keys, ivs and key_status are host
 * arrays with one entry per stream (32 bytes, 16 bytes, one uint32) as
 * chipc_stream_keys_dev wrote them; they are looked at for format 15 only,
 * and key_status may be NULL (all 0).
 *
 * WHAT A READ GUARANTEES.  With status 0 and !(d_vouch[r] & CHIPV_UNVOUCHED)
 * (with CHIPV_STRICT: status 0 alone), the compressed bytes behind the range
 * were hashed against the stream's root, each frame's header agrees with the
 * index, and each block matches its CRC-32C.  That the f-th index entry IS the
 * f-th frame is proven by layers 1 and 2, not by a read: an index that is
 * self-consistent but wrong (one that starts at the second of two full frames
 * of equal size and calls it the first: it ascends, ends at L and agrees with
 * that frame's header) reads status 0 and the other frame's bytes.  At
 * level 15 a wrong key gives garbage headers and status 16, unlike
 * carbonado_hip_cread.h; the GCM tag is NOT checked, as there.
 * Reads with a proven index survive shard damage as vouched reads do.  The
 * index BUILD (layer 2) does not survive damage to a header's primary copy:
 * its walk reads the primary copy unverified.  Such a stream ends with 5, 7 or
 * 16 and a vouch bit (or, where the damage lies in bytes the walk does not use,
 * with 0, a vouch bit and the right index); the caller scrubs
 * (chipr_scrub_ragged_dev) and calls again.
 *
 * Constant time, as in carbonado_hip_cread.h: on the device no load or store
 * address and no branch depends on a key, a round key, J0 or keystream.  Frame
 * lengths, types and CRCs are plaintext of the object and DO drive addresses
 * and branches, as they already do in the snappy stage of a level-15 decode.
 * Key material lives in the key regions of a call's scratch; each is
 * overwritten with zeros by the operation enqueued directly behind the last
 * kernel that reads it (the walk, the keystream kernels), and the host copies
 * are wiped as in carbonado_hip_cread.h.
 */
#ifndef CARBONADO_HIP_FREAD_H
#define CARBONADO_HIP_FREAD_H

#include "carbonado_hip_cread.h"
#include "carbonado_hip_snap.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define CHIPF_API __attribute__((visibility("default")))
#else
#define CHIPF_API
#endif

#define CHIPF_ABI_VERSION 1

CHIPF_API int chipf_abi_version(void);

/* ---- 1. an index proven against the stream --------------------------------------
 * Bytes of device scratch chipf_verify_index_dev or chipf_frame_index_dev needs
 * for nstreams streams and nentries index entries in all (the sum of
 * nframes[s] + 1, or of idx_cap[s]): a multiple of 16, growing with either.
 * 0 for nstreams >= 2^31 or nentries >= 2^30.  Host only. */
CHIPF_API uint64_t chipf_index_scratch_len(uint64_t nstreams, uint64_t nentries);

/* Proves the index frame_off[idx_off[s] .. idx_off[s] + nframes[s]] of every
 * stream (the stream arguments of chipv_read_ranges_dev) against the stream.
 * Enqueues its work and waits for nothing: (1) one strict vouched read
 * (CHIPV_STRICT) into staging rows of the scratch, of the 10 identifier bytes
 * and, for every frame f, of frame-stream bytes [off[f], min(off[f] + 12, L)):
 * header, CRC and the up to 3 varint bytes a length <= 65536 takes; (2) at 15,
 * the keystream over those ranges, gated on the read's status; (3) the chain
 * kernel, one wave per stream.  Launches: the vouched read's (at most 8), 2
 * for the keystream, 1, whatever the batch.  Written, device arrays with one
 * entry per stream:
 * d_index_status[s]: 0 exactly when the identifier is right, every header has
 *   type 0 or 1, off[f] + 4 + clen == off[f + 1], the last chunk ends at L and
 *   the uncompressed lengths (type 1: clen - 4; type 0: the varint) are 65536
 *   but for the last, which has 1..65536 (for L = 0: nframes = 0 and the entry
 *   0); the read's 5, else 7, if a header could not be served; else
 *   CHIP_ERR_SNAP (16) if some link is wrong; else 11 for a well-formed chain
 *   that is not canonical.  key_status[s] where that is non-zero, and
 *   CHIP_ERR_ZFEC (7) for a stream whose chunk_len or padding does not fit:
 *   no work is done for such a stream.
 * d_plain_len[s] (uint64): the plaintext's length for status 0, else 0.
 * d_index_vouch[s]: the OR of the vouch words of its header reads.  A caller
 *   who sees 16 together with CHIPV_VOUCHED knows that a header's primary copy
 *   is damaged.
 * Host-decided, in this order: nstreams == 0 is CHIP_OK and touches nothing.
 * CHIP_ERR_INVALID_ARG for a format other than 14 and 15; for a NULL keys or
 * ivs at 15; for a NULL d_streams, in_off, in_len, padding, chunk_len,
 * frame_off, idx_off, nframes, d_index_status, d_plain_len, d_index_vouch or
 * d_scratch; for nstreams >= 2^31, an nframes[s] >= 2^30 or 2^30 entries in
 * all; for a stream address that is not 8-B aligned or a d_scratch that is not
 * 16-B aligned; for an entry above 2^53; for scratch_len below
 * chipf_index_scratch_len(nstreams, sum of nframes[s] + 1).  Then
 * CHIP_ERR_BAO_TRUNCATED, CHIP_ERR_HASH_DECODE (a NULL d_hash),
 * CHIP_ERR_NO_DEVICE. */
CHIPF_API int chipf_verify_index_dev(uint8_t format, const uint8_t *keys, const uint8_t *ivs,
                                     const uint32_t *key_status, const uint8_t *d_streams, const uint64_t *in_off,
                                     const uint64_t *in_len, const uint8_t *d_hash, const uint32_t *padding,
                                     const uint32_t *chunk_len, uint64_t nstreams, const uint64_t *frame_off,
                                     const uint64_t *idx_off, const uint64_t *nframes, uint32_t *d_index_status,
                                     uint64_t *d_plain_len, uint32_t *d_index_vouch, void *d_scratch,
                                     uint64_t scratch_len, void *stream);

/* ---- 2. the index of resident streams ----------------------------------------------
 * Builds and proves the index of every stream.  A walk kernel, one lane per
 * stream, follows the chunk headers serially: it reads the primary copy
 * straight from the stream at the stream's geometry, unverified, and at 15
 * decrypts the 12 bytes of each hop with one lane-local evaluation of the two
 * keystream blocks they span.  Every hop advances by at least 8 bytes and the
 * walk stops at L, at a header that is not a canonical data chunk, or keeps
 * counting without writing past idx_cap[s] entries: a corrupt stream ends in a
 * status, never in a wait.  The offsets come back in one gathered copy and THE
 * CALL WAITS ONCE; layer 1 then runs over them, and the call waits a second
 * time for its three words per stream.  Written, all host memory:
 * frame_off[idx_off[s] ..]: the entries (nframes[s] + 1 of them for status 0);
 * nframes[s]; index_status[s], plain_len[s] and index_vouch[s] as layer 1
 * gives them, and before that: CHIP_ERR_BUFFER_TOO_SMALL (2) for an idx_cap[s]
 * below nframes[s] + 1, with nframes[s] the number of frames found, so that
 * nframes[s] + 1 entries are needed; 11 or 16 as the walk found it (layer 1
 * still reads the header the walk stopped at, so that index_vouch[s] tells
 * damage from a stream that was never canonical, and its 5 or 7 stand).
 * plain_len[s] is 0 unless the status is 0.
 * The host outputs are valid only when the call returns CHIP_OK: a call that
 * fails behind its host checks (CHIP_ERR_DEVICE) may have written some of
 * frame_off and nframes and none of the three words, and the caller must use
 * none of them.
 * Host-decided, in this order: as chipf_verify_index_dev, with idx_cap, the
 * five host output arrays and chipf_index_scratch_len(nstreams, sum of
 * idx_cap[s]) in the place of nframes, the device arrays and its scratch
 * length; an idx_cap[s] >= 2^30 is refused. */
CHIPF_API int chipf_frame_index_dev(uint8_t format, const uint8_t *keys, const uint8_t *ivs,
                                    const uint32_t *key_status, const uint8_t *d_streams, const uint64_t *in_off,
                                    const uint64_t *in_len, const uint8_t *d_hash, const uint32_t *padding,
                                    const uint32_t *chunk_len, uint64_t nstreams, uint64_t *frame_off,
                                    const uint64_t *idx_off, const uint64_t *idx_cap, uint64_t *nframes,
                                    uint32_t *index_status, uint64_t *plain_len, uint32_t *index_vouch,
                                    void *d_scratch, uint64_t scratch_len, void *stream);

/* ---- 3. the read ---------------------------------------------------------------------
 * Requests are in PLAINTEXT bytes: the content of request r is plaintext
 * [start[r], min(plain_len[s], start[r] + len[r])) of stream s = req_stream[r].
 * It covers frames f0 = start / 65536 .. f1 = (end - 1) / 65536.
 *
 * Host only: content offsets (multiples of align, itself a multiple of 16) and
 * lengths of every request, their total, and what chipf_read_scratch_len wants:
 * nseg, the number of (request, frame) work items; stage_total, the bytes of
 * the 16-B aligned staging rows (frame-stream bytes [off[f0], off[f1 + 1]) per
 * request); vseg, the segments of the vouched read of those rows.  The output
 * pointers may be NULL.  index_status: as chipf_read_ranges_dev takes it, or
 * NULL (all 0): a request of a stream whose word is not zero claims its
 * content range and counts nothing else, and that stream's index is not
 * looked at.  CHIP_ERR_INVALID_ARG for a format other than 14 and
 * 15, an align that is 0 or no multiple of 16, a NULL input array with
 * nreq > 0, a req_stream[r] >= nstreams, a start or len above 2^53, or an
 * index that does not fit (entries that do not ascend, a last entry that is
 * not L, a plain_len outside (65536 (nframes - 1), 65536 nframes]) of a
 * stream whose index_status is 0. */
CHIPF_API int chipf_read_layout(uint8_t format, const uint32_t *chunk_len, const uint32_t *padding,
                                const uint32_t *index_status, const uint64_t *frame_off, const uint64_t *idx_off,
                                const uint64_t *nframes, const uint64_t *plain_len, uint64_t nstreams,
                                const uint32_t *req_stream,
                                const uint64_t *start, const uint64_t *len, uint64_t nreq, uint64_t align,
                                uint64_t *content_off, uint64_t *content_len, uint64_t *content_total, uint64_t *nseg,
                                uint64_t *stage_total, uint64_t *vseg);

/* Bytes of device scratch a read needs (the numbers of chipf_read_layout): a
 * multiple of 16, growing with each.  0 for nreq or nseg >= 2^31.  Host only. */
CHIPF_API uint64_t chipf_read_scratch_len(uint64_t nreq, uint64_t nseg, uint64_t stage_total, uint64_t vseg,
                                          uint64_t nstreams);

/* The plaintext of every request.  index_status: host, one word per stream as
 * layer 1 or 2 gave it, or NULL (all 0).  The call (a) runs the vouched read of
 * frame-stream bytes [off[f0], off[f1 + 1]) (+97 at level 15) into the
 * request's staging row, with the caller's flags; (b) at 15, runs the
 * keystream over the row with pos = off[f0], gated on the read's status, and
 * zeroes the key region; (c) runs the block kernel, one wave per (request,
 * frame): it checks the staged header against the index (type 0 or 1; clen ==
 * off[f + 1] - off[f] - 4; the uncompressed length 65536, or the last frame's),
 * decodes a compressed block into 64 KiB of LDS, checks the masked CRC-32C
 * over it (over the staged bytes for a raw chunk) and stores only
 * [max(start, 65536 f), min(end, 65536 (f + 1))) into the content range, at any
 * byte address, with 16-B stores where aligned; (d) runs the finish kernel,
 * one workgroup per request: if any frame is bad it writes zeros over the
 * content range and sets status 16.  Nothing is waited for: the at most 8
 * launches of the vouched read, 2 of the keystream, 2 of (c) and (d).
 * d_used and d_vouch are the vouched read's.  d_status[r] is index_status of
 * its stream where that is non-zero: such a request does no work, gets zeros
 * and d_used[r] = d_vouch[r] = 0; otherwise it is the read's 5 or 7, else 16,
 * else 0.  content_len[r] (host, written) is the layout's whatever the status.
 * Content is all or nothing per request: the exact plaintext for status 0,
 * zeros otherwise; no other byte of d_content is touched (content_off[r] may
 * be any byte offset), nothing past scratch_len in d_scratch, and d_streams is
 * never written.  An empty request, or one at or beyond plain_len, has status
 * 0 and no content.
 * Host-decided, in this order: nreq == 0 is CHIP_OK and touches nothing.
 * CHIP_ERR_INVALID_ARG for a NULL keys or ivs at 15 or a NULL frame_off,
 * idx_off, nframes or plain_len; then for a NULL array or buffer of
 * chipv_read_ranges_dev's list (d_content only where some request has
 * content); for a format other than 14 and 15; for a bit of flags other than
 * CHIPV_STRICT; for nreq or nstreams >= 2^31; for a req_stream[r] >= nstreams
 * or a start or len above 2^53; for an index that does not fit
 * (chipf_read_layout), of a stream whose index_status is 0; then everything
 * chipv_read_ranges_dev still refuses (a stream address that is not 8-B
 * aligned, a d_scratch that is not 16-B aligned); for content ranges that
 * overlap; for scratch_len below chipf_read_scratch_len of this call's
 * numbers.  Then CHIP_ERR_BAO_TRUNCATED, CHIP_ERR_HASH_DECODE,
 * CHIP_ERR_NO_DEVICE. */
CHIPF_API int chipf_read_ranges_dev(uint8_t format, const uint8_t *keys, const uint8_t *ivs,
                                    const uint32_t *index_status, const uint64_t *frame_off, const uint64_t *idx_off,
                                    const uint64_t *nframes, const uint64_t *plain_len, const uint8_t *d_streams,
                                    const uint64_t *in_off, const uint64_t *in_len, const uint8_t *d_hash,
                                    const uint32_t *padding, const uint32_t *chunk_len, uint64_t nstreams,
                                    const uint32_t *req_stream, const uint64_t *start, const uint64_t *len,
                                    uint64_t nreq, uint8_t *d_content, const uint64_t *content_off,
                                    uint64_t *content_len, uint32_t *d_status, uint32_t *d_used, uint32_t *d_vouch,
                                    uint32_t flags, void *d_scratch, uint64_t scratch_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CARBONADO_HIP_FREAD_H */
