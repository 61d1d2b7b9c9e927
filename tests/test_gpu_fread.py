"""Plaintext ranged reads of level-14 and level-15 streams
(include/carbonado_hip_fread.h): the frame index against a Python walk of the
host's frame stream (chip_snap_compress, which the device's streams equal), its
proof against the stream, and the reads against slices of the test's own
plaintexts, encoded by encode_ragged_snap (at 15 with injected ephemeral secrets
and nonces).  Every comparison of content is of whole buffers over a canary
fill, so the bytes outside the ranges are checked too."""
import functools

import numpy as np
import pytest
import torch

import snap_data as SD  # tests/snap_data.py (tests/ is on sys.path under pytest)
from read_world import PlainStreams, dev, up16

pytestmark = pytest.mark.gpu

TOO_SMALL, HASH, ZFEC, UNSUPPORTED, SNAP = 2, 5, 7, 11, 16
VOUCHED = 1
FRAME = 65536
SECRET = bytes(range(1, 33))
# lengths around one and two frames, and one of four frames; "mix": the compressible generator of tools/snap_bench.py
SIZES = [0, 1, 65535, 65536, 65537, 131072, 131077, 200003]
KINDS = ["random", "mix", "random", "mix", "random", "random", "mix", "mixed"]
TWO_RAW, BIG = 5, 7   # two full raw frames of equal size; the stream the damage cases use
FORMATS = (14, 15)


def plaintexts():
    rng = np.random.default_rng(77)
    out = []
    for i, (n, kind) in enumerate(zip(SIZES, KINDS)):
        if kind == "random":
            out.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif kind == "mix":
            out.append(SD.mix(n, 40, 900 + i))
        else:  # compressible, then random: a compressed frame, a frame of both, raw frames
            out.append(SD.mix(100000, 40, 900 + i) + rng.integers(0, 256, n - 100000, dtype=np.uint8).tobytes())
    return out


def walk(frame: bytes):
    """The frame index of a canonical frame stream, and its plaintext length."""
    if not frame:
        return [0], 0
    assert frame[:10] == b"\xff\x06\x00\x00sNaPpY"
    pos, off, plain = 10, [], 0
    while pos < len(frame):
        ty, clen = frame[pos], int.from_bytes(frame[pos + 1:pos + 4], "little")
        assert ty in (0, 1)
        if ty == 1:
            ulen = clen - 4
        else:
            ulen, shift = 0, 0
            for b in frame[pos + 8:pos + 11]:
                ulen |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
        off.append(pos)
        plain += ulen
        pos += 4 + clen
    assert pos == len(frame)
    return off + [pos], plain


class Streams(PlainStreams):
    def __init__(self, fmt):
        from carbonado_amd import device as D
        from carbonado_amd import encoding as E
        self.fmt, self.count, self.shift = fmt, len(SIZES), 97 if fmt == 15 else 0
        self.pt = plaintexts()
        self.frames = [E.snap(p) for p in self.pt]
        self.index = [walk(f)[0] for f in self.frames]
        assert [walk(f)[1] for f in self.frames] == SIZES
        # the inputs must exercise both chunk types and both single- and multi-frame objects
        types = {f[o] for f, idx in zip(self.frames, self.index) for o in idx[:-1]}
        assert types == {0, 1} and {len(i) - 1 for i in self.index} >= {0, 1, 2, 4}
        assert [self.frames[BIG][o] for o in self.index[BIG][:-1]] == [0, 0, 1, 1]
        rng = np.random.default_rng(78)
        self.pub = E.public_key(SECRET)
        self.inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(),
                        rng.integers(0, 256, 16, dtype=np.uint8).tobytes()) for _ in SIZES]
        in_off, plain = self.place_plain(SIZES)
        self.off, self.cap, total = D.snap_encode_layout(fmt, SIZES, 256)
        self.make_outputs(total, self.count)
        self.olen, info = D.encode_ragged_snap(fmt, dev(plain), in_off, SIZES, self.out, self.off, self.hashes,
                                               D.snap_ragged_scratch(fmt, SIZES), pubkey=self.pub if fmt == 15 else None,
                                               inject=self.inject if fmt == 15 else None)
        torch.cuda.synchronize()
        self.pads, self.cls = [i.padding_len for i in info], [i.chunk_len for i in info]
        assert [4 * c - p - self.shift for c, p in zip(self.cls, self.pads)] == [len(f) for f in self.frames]
        self.keys = self.ivs = None
        if fmt == 15:
            self.keys, self.ivs, kstat = D.stream_keys(SECRET, self.out, self.off, self.olen, self.hashes, self.pads,
                                                       self.cls, D.stream_keys_scratch(self.count))
            assert kstat.tolist() == [0] * self.count
        # the true index as the calls take it: entries with a gap between the streams
        self.nframes = [len(i) - 1 for i in self.index]
        self.idx_off, at = [], 3
        for i in self.index:
            self.idx_off.append(at)
            at += len(i) + 2
        self.frame_off = np.full(at, 0x7777777777, dtype=np.uint64)
        for o, i in zip(self.idx_off, self.index):
            self.frame_off[o:o + len(i)] = i

    # ---- damage
    def stream_pos(self, s, x):
        """Where byte x of stream s's content (object byte x, or shard i's column c at i C + c) lies in the stream."""
        return self.chunk_pos(s, x // 1024, x % 1024)

    def damaged(self, s, content_bytes):
        return self.flipped(self.stream_pos(s, x) for x in content_bytes)

    # ---- the calls
    def build(self, caps=None, out=None, keys=None):
        from carbonado_amd import device as D
        caps = [n + 1 for n in self.nframes] if caps is None else caps
        return D.frame_index(self.fmt, self.out if out is None else out, self.off, self.olen, self.hashes, self.pads,
                             self.cls, self.idx_off, caps, D.frame_index_scratch(self.count, sum(caps)),
                             keys=self.keys if keys is None else keys, ivs=self.ivs)

    def verify(self, frame_off=None, nframes=None, out=None):
        from carbonado_amd import device as D
        nframes = self.nframes if nframes is None else nframes
        st, vo = (torch.full((self.count,), 0x7777, dtype=torch.int32, device="cuda") for _ in range(2))
        plain = torch.full((self.count,), -1, dtype=torch.int64, device="cuda")
        D.verify_frame_index(self.fmt, self.out if out is None else out, self.off, self.olen, self.hashes, self.pads,
                             self.cls, self.frame_off if frame_off is None else frame_off, self.idx_off, nframes, st,
                             plain, vo, D.frame_index_scratch(self.count, sum(n + 1 for n in nframes)), keys=self.keys,
                             ivs=self.ivs)
        torch.cuda.synchronize()
        return st.cpu().tolist(), plain.cpu().tolist(), vo.cpu().tolist()

    def read(self, reqs, out=None, flags=0, frame_off=None, nframes=None, plain_len=None, index_status=None, keys=None):
        """(content image, status, used, vouch, content_off, content_len) of read_frame_ranges; the content
        ranges lie at every residue mod 16 with canary bytes between them."""
        from carbonado_amd import device as D
        rs, start, length = [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]
        frame_off = self.frame_off if frame_off is None else frame_off
        nframes = self.nframes if nframes is None else nframes
        plain_len = SIZES if plain_len is None else plain_len
        _, clen, _, nseg, stage, vseg = D.frame_read_layout(self.fmt, self.cls, self.pads, frame_off, self.idx_off,
                                                            nframes, plain_len, rs, start, length,
                                                            index_status=index_status)
        coff, at = [], 5
        for r, n in enumerate(clen):
            at += (r * 7) % 16 + 1
            coff.append(at)
            at += n
        content = torch.full((at + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        st, used, vouch = (torch.full((len(reqs),), 0x7777, dtype=torch.int32, device="cuda") for _ in range(3))
        got = D.read_frame_ranges(self.fmt, self.out if out is None else out, self.off, self.olen, self.hashes,
                                  self.pads, self.cls, frame_off, self.idx_off, nframes, plain_len, rs, start, length,
                                  content, coff, st, used, vouch,
                                  D.frame_read_scratch(len(reqs), nseg, stage, vseg, self.count), flags=flags,
                                  keys=self.keys if keys is None else keys, ivs=self.ivs, index_status=index_status)
        torch.cuda.synchronize()
        assert got == clen
        return content.cpu().numpy(), st.cpu().tolist(), used.cpu().tolist(), vouch.cpu().tolist(), coff, clen


@functools.lru_cache(maxsize=None)
def streams(fmt) -> Streams:
    return Streams(fmt)


def requests():
    rq = []
    for s, P in enumerate(SIZES):
        rq += [(s, 0, P), (s, 0, 1), (s, max(P - 1, 0), 1), (s, P, 10), (s, P + 5, 10), (s, min(3, P), 0),
               (s, max(P - 10, 0), 100)]
    rq += [(BIG, 1000, 4096), (BIG, FRAME - 20, 40), (BIG, FRAME, FRAME), (BIG, 2 * FRAME - 1, 2),
           (BIG, FRAME + 17, 2 * FRAME), (BIG, 3 * FRAME - 100, 5000), (6, FRAME - 1, 6), (6, 2 * FRAME, 5),
           (4, FRAME, 1), (TWO_RAW, 12345, FRAME), (3, 4096, 4096)]
    rq += [(BIG, 70000 + 17 * k, 33 + k) for k in range(16)]
    return rq


# ---- the index ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_index_is_the_python_walk(gpu, fmt):
    s = streams(fmt)
    frame_off, nframes, status, plain, vouch = s.build()
    assert status.tolist() == [0] * s.count and vouch.tolist() == [0] * s.count
    assert nframes.tolist() == s.nframes and plain.tolist() == SIZES
    for o, i in zip(s.idx_off, s.index):
        assert frame_off[o:o + len(i)].tolist() == i
    # capacity one short: 2 and the number of frames found, the other streams as before
    caps = [n + 1 for n in s.nframes]
    caps[BIG] -= 1
    caps[0] -= 1
    frame_off, nframes, status, plain, vouch = s.build(caps=caps)
    assert status.tolist() == [TOO_SMALL if o in (0, BIG) else 0 for o in range(s.count)]
    assert nframes.tolist() == s.nframes and plain.tolist() == [0 if o in (0, BIG) else n for o, n in enumerate(SIZES)]
    assert frame_off[s.idx_off[BIG]:s.idx_off[BIG] + caps[BIG]].tolist() == s.index[BIG][:-1]


@pytest.mark.parametrize("fmt", FORMATS)
def test_verify_accepts_the_true_index_and_nothing_else(gpu, fmt):
    s = streams(fmt)
    assert s.verify() == ([0] * s.count, SIZES, [0] * s.count)
    fo, nf = s.frame_off.copy(), list(s.nframes)
    fo[s.idx_off[BIG] + 1] += 1                                    # an entry off by one
    a = s.idx_off[TWO_RAW]
    fo[a], fo[a + 1] = fo[a + 1], fo[a]                            # two entries exchanged: the lengths break
    b = s.idx_off[6]
    fo[b + 1:b + 3] = fo[b + 2:b + 4]                              # a frame dropped
    nf[6] -= 1
    fo[s.idx_off[1] + 1] -= 1                                      # a last entry that is not L
    status, plain, vouch = s.verify(frame_off=fo, nframes=nf)
    bad = {BIG, TWO_RAW, 6, 1}
    assert status == [SNAP if o in bad else 0 for o in range(s.count)]
    assert plain == [0 if o in bad else n for o, n in enumerate(SIZES)] and vouch == [0] * s.count


def test_a_stream_that_is_not_canonical_gets_11(gpu):
    from carbonado_amd import device as D
    content = bytes(range(200)) * 3
    ident = b"\xff\x06\x00\x00sNaPpY"
    objs = [ident + SD.chunk(0x80, b"pad") + SD.data_chunk(content),          # a skippable chunk
            ident + SD.data_chunk(content[:100]) + SD.data_chunk(content),    # a short inner block
            ident + SD.data_chunk(content) + ident,                           # a repeated identifier
            ident + SD.data_chunk(content)]                                   # canonical
    index = [[10, 17, len(objs[0])], [10, 118, len(objs[1])], [10, 618, len(objs[2])], [10, len(objs[3])]]
    sizes = [len(o) for o in objs]
    in_off = [1024 * i for i in range(4)]
    inp = np.zeros(4096, dtype=np.uint8)
    for o, a in zip(objs, in_off):
        inp[a:a + len(o)] = np.frombuffer(o, dtype=np.uint8)
    off, _, total = D.ragged_layout(12, sizes, 256)
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    hashes = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
    olen, info = D.encode_ragged(12, dev(inp), in_off, sizes, out, off, hashes, D.ragged_scratch(12, sizes))
    pads, cls = [i.padding_len for i in info], [i.chunk_len for i in info]
    idx_off = [0, 4, 8, 12]
    frame_off = np.zeros(16, dtype=np.uint64)
    for a, i in zip(idx_off, index):
        frame_off[a:a + len(i)] = i
    st, vo = (torch.full((4,), 0x7777, dtype=torch.int32, device="cuda") for _ in range(2))
    plain = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    D.verify_frame_index(14, out, off, olen, hashes, pads, cls, frame_off, idx_off, [2, 2, 2, 1], st, plain, vo,
                         D.frame_index_scratch(4, 11))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, 0] and plain.cpu().tolist() == [0, 0, 0, 600]
    got = D.frame_index(14, out, off, olen, hashes, pads, cls, idx_off, [4] * 4, D.frame_index_scratch(4, 16))
    assert got[2].tolist() == [UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, 0] and got[3].tolist() == [0, 0, 0, 600]
    assert got[0][12:14].tolist() == index[3] and got[4].tolist() == [0] * 4


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_damaged_header_fails_the_build_until_scrubbed_and_not_the_proof(gpu, fmt):
    from carbonado_amd import device as D
    s = streams(fmt)
    x = s.shift + s.index[BIG][1] + 1          # the low length byte of frame 1's header, in its primary copy
    assert x < 4 * s.cls[BIG]
    bad = s.damaged(BIG, [x])
    frame_off, nframes, status, plain, vouch = s.build(out=bad)
    assert status[BIG] in (SNAP, HASH, ZFEC) and vouch[BIG] & VOUCHED and plain[BIG] == 0
    assert [status[o] for o in range(s.count) if o != BIG] == [0] * (s.count - 1)
    # the proof of the true index survives the damage, and says that a header was rebuilt
    st, pl, vo = s.verify(out=bad)
    assert st == [0] * s.count and pl == SIZES and vo == [VOUCHED if o == BIG else 0 for o in range(s.count)]
    # scrubbed where it lies, the build gives the true index again
    res = D.scrub_ragged(bad, s.off, s.olen, s.hashes, s.pads, s.cls, bad, s.off, D.scrub_ragged_scratch(s.olen))
    assert res[BIG] == 0
    frame_off, nframes, status, plain, vouch = s.build(out=bad)
    assert status.tolist() == [0] * s.count and vouch.tolist() == [0] * s.count and plain.tolist() == SIZES
    assert frame_off[s.idx_off[BIG]:s.idx_off[BIG] + 5].tolist() == s.index[BIG]


# ---- the reads -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_plaintext_ranges_of_intact_streams(gpu, fmt):
    s = streams(fmt)
    reqs = requests()
    content, status, used, vouch, coff, clen = s.read(reqs)
    assert status == [0] * len(reqs) and vouch == [0] * len(reqs)
    assert clen == [len(s.pt[o][a:a + n]) for o, a, n in reqs]
    assert np.array_equal(content, s.want(reqs, coff, content.size))
    assert {c % 16 for c, n in zip(coff, clen) if n} == set(range(16))
    # under CHIPV_STRICT an intact stream reads the same
    strict = s.read(reqs[-20:], flags=1)
    assert strict[1] == [0] * 20 and np.array_equal(strict[0], s.want(reqs[-20:], strict[4], strict[0].size))


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_read_equals_the_full_decode_sliced(gpu, fmt):
    from carbonado_amd import device as D
    s = streams(fmt)
    pitch = up16(max(SIZES))
    back = torch.zeros(s.count * pitch, dtype=torch.uint8, device="cuda")
    got = torch.zeros(s.count, dtype=torch.int64, device="cuda")
    st = torch.zeros(s.count, dtype=torch.int32, device="cuda")
    ooff = [o * pitch for o in range(s.count)]
    D.decode_ragged_snap(fmt, s.out, s.off, s.olen, s.hashes, s.pads, back, ooff, [pitch] * s.count, got, st,
                         D.snap_ragged_scratch(fmt, s.olen, [pitch] * s.count), secret_key=SECRET if fmt == 15 else None)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * s.count and got.cpu().tolist() == SIZES
    host = back.cpu().numpy()
    decoded = [host[o:o + n].tobytes() for o, n in zip(ooff, SIZES)]
    reqs = requests()
    content, status, _, _, coff, _ = s.read(reqs)
    assert status == [0] * len(reqs) and np.array_equal(content, s.want(reqs, coff, content.size, pt=decoded))


def _big_requests(s):
    return [(BIG, 2 * FRAME + 1000, 300), (BIG, 10, 100), (BIG, 3 * FRAME + 5, 50), (3, 100, 4000), (BIG, SIZES[BIG] - 1, 1)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_damaged_window_is_rebuilt_and_vouched_for_or_fails_alone(gpu, fmt):
    s = streams(fmt)
    reqs = _big_requests(s)
    C = s.cls[BIG]
    x = s.shift + s.index[BIG][2] + 2000          # inside frame 2's raw bytes, which request 0 alone stages
    p, col = x // C, x % C
    content, status, used, vouch, coff, _ = s.read(reqs, out=s.damaged(BIG, [x]))
    assert status == [0] * 5 and vouch == [VOUCHED, 0, 0, 0, 0]
    assert bin(used[0]).count("1") == 4 and not used[0] & (1 << p)
    assert np.array_equal(content, s.want(reqs, coff, content.size))
    # the same chunk damaged in five shards (its primary and the four parity shards, which no other request
    # reads directly): status 7 and zeros, the stream's other requests still served
    shards = [p, 4, 5, 6, 7]
    content, status, used, vouch, coff, _ = s.read(reqs, out=s.damaged(BIG, [i * C + col for i in shards]))
    assert status == [ZFEC, 0, 0, 0, 0] and used[0] == 0 and vouch[0] == 0
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0}))


@pytest.mark.parametrize("fmt", FORMATS)
def test_requests_of_a_stream_without_an_index_and_of_a_wrong_index(gpu, fmt):
    s = streams(fmt)
    reqs = _big_requests(s) + [(6, 5, 10), (6, 0, 0)]
    # a non-zero index_status: that status, zeros, no work; the stream's index is not looked at
    istat = [0] * s.count
    istat[BIG], istat[6] = UNSUPPORTED, HASH
    fo = s.frame_off.copy()
    fo[s.idx_off[BIG]:s.idx_off[BIG] + 5] = 0
    content, status, used, vouch, coff, clen = s.read(reqs, frame_off=fo, index_status=istat)
    assert status == [UNSUPPORTED] * 3 + [0, UNSUPPORTED, HASH, HASH]
    assert [u for r, u in enumerate(used) if r != 3] == [0] * 6 and vouch == [0] * 7
    assert clen == [300, 100, 50, 4000, 1, 10, 0]
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0, 1, 2, 4, 5, 6}))
    # an index with one length wrong: 16 and zeros for the frames on either side of the entry, the others served
    fo = s.frame_off.copy()
    fo[s.idx_off[BIG] + 2] += 1
    reqs = [(BIG, 2 * FRAME + 1000, 300), (BIG, FRAME + 7, 9), (BIG, 10, 100), (BIG, 3 * FRAME + 5, 50),
            (BIG, FRAME - 5, 10), (BIG, 0, SIZES[BIG])]
    content, status, used, vouch, coff, clen = s.read(reqs, frame_off=fo)
    assert status == [SNAP, SNAP, 0, 0, SNAP, SNAP]
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0, 1, 4, 5}))


def test_a_wrong_key_at_15_gives_16(gpu):
    from carbonado_amd import device as D
    s = streams(15)
    keys, ivs, kstat = D.stream_keys(bytes(range(3, 35)), s.out, s.off, s.olen, s.hashes, s.pads, s.cls,
                                     D.stream_keys_scratch(s.count))
    assert kstat.tolist() == [0] * s.count and not np.array_equal(keys, s.keys)
    reqs = [(3, 100, 4000), (BIG, 0, 1000), (BIG, FRAME - 1, 2), (1, 0, 1), (0, 0, 5)]
    content, status, used, vouch, coff, clen = s.read(reqs, keys=keys)
    assert status == [SNAP, SNAP, SNAP, SNAP, 0] and clen == [4000, 1000, 2, 1, 0]
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0, 1, 2, 3}))
    # and the index build under it finds no identifier
    assert s.build(keys=keys)[2].tolist() == [0] + [SNAP] * (s.count - 1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_pinned_limit_a_self_consistent_wrong_index(gpu, fmt):
    """A read proves each frame against the index, not the index against the
    stream: an index that starts at the second of two equal-sized full frames
    and calls it the only one ascends, ends at L and agrees with that frame's
    header, so the read gives status 0 and the other frame's bytes.  Layer 1
    refuses the same index."""
    s = streams(fmt)
    assert s.index[TWO_RAW][1] - s.index[TWO_RAW][0] == s.index[TWO_RAW][2] - s.index[TWO_RAW][1] == FRAME + 8
    fo, nf, pl = s.frame_off.copy(), list(s.nframes), list(SIZES)
    a = s.idx_off[TWO_RAW]
    fo[a:a + 2] = s.index[TWO_RAW][1:]
    nf[TWO_RAW], pl[TWO_RAW] = 1, FRAME
    reqs = [(TWO_RAW, 100, 500), (TWO_RAW, FRAME - 3, 10)]
    content, status, used, vouch, coff, clen = s.read(reqs, frame_off=fo, nframes=nf, plain_len=pl)
    assert status == [0, 0] and clen == [500, 3]
    other = [(TWO_RAW, FRAME + 100, 500), (TWO_RAW, 2 * FRAME - 3, 3)]
    assert np.array_equal(content, s.want(other, coff, content.size))
    assert s.verify(frame_off=fo, nframes=nf)[0][TWO_RAW] == SNAP
