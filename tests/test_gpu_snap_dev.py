"""The snappy framing format over device-resident objects
(include/carbonado_hip_snap.h) against the library's own host stage
(chip_snap_compress / chip_snap_decompress) and the oracle's C restatement
(c_snap_compress / c_snap_decompress / orc_encode_full): compressed streams
byte for byte, since a stream's bao hash is the object's name.  Every
comparison is of whole buffers, so the bytes between the ranges (a canary
fill) are checked with the ranges themselves.  The inputs are required to
exercise every kind of chunk, tag and header before anything is compared."""
import ctypes
import math

import numpy as np
import pytest
import torch

import snap_data as SD
from read_world import dev, up16

pytestmark = pytest.mark.gpu

OK, TOO_SMALL, BAO, MANY, SNAP, ECIES = 0, 2, 5, 11, 16, 17
SECRET = bytes(range(1, 33))


def host_snap(data: bytes) -> bytes:
    import carbonado_amd as ca
    return ca.encoding.snap(data)


def host_unsnap(stream: bytes, cap: int):
    """(status, length, bytes) of chip_snap_decompress for these bytes and this capacity."""
    from carbonado_amd import _lib
    a = np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, dtype=np.uint8)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    olen = ctypes.c_uint64(0)
    st = _lib.lib().chip_snap_decompress(a.ctypes.data, len(stream), out.ctypes.data, cap, ctypes.byref(olen))
    return st, olen.value, out[:olen.value].tobytes() if st == OK else b""


def run_snap(datas, fill=0xA5):
    """One call over `datas`; object o's stream at residue o % 16.  Returns
    (out image, out_off, out_len, the canary image with nothing in it)."""
    from carbonado_amd import device as D
    lens = [len(d) for d in datas]
    in_off, pos = [], 0
    for n in lens:
        in_off.append(pos)
        pos += up16(n)
    inp = np.full(pos + 16, 0x11, dtype=np.uint8)
    for d, off in zip(datas, in_off):
        inp[off:off + len(d)] = np.frombuffer(d, dtype=np.uint8)
    out_off, pos = [], 0
    for o, n in enumerate(lens):
        out_off.append(up16(pos) + o % 16)
        pos = out_off[-1] + D.snap_max_len(n)
    out = torch.full((pos + 64,), fill, dtype=torch.uint8, device="cuda")
    out_len = torch.full((len(datas),), -1, dtype=torch.int64, device="cuda")
    D.snap_ragged(dev(inp), in_off, lens, out, out_off, out_len, D.snap_scratch(lens))
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_off, out_len.cpu().tolist(), np.full(pos + 64, fill, dtype=np.uint8)


def run_unsnap(streams, caps, fill=0x5A):
    """One call over `streams` at odd input addresses.  Returns (out image,
    out_off, out_len, status)."""
    from carbonado_amd import device as D
    in_off, pos = [], 1
    for s in streams:
        in_off.append(pos)
        pos += len(s) + (2 if len(s) % 2 == 0 else 1)   # the next address is odd again
    inp = np.full(pos + 16, 0x33, dtype=np.uint8)
    for s, off in zip(streams, in_off):
        inp[off:off + len(s)] = np.frombuffer(s, dtype=np.uint8)
    out_off, pos = [], 0
    for c in caps:
        out_off.append(pos)
        pos += up16(c) + 16
    out = torch.full((pos + 64,), fill, dtype=torch.uint8, device="cuda")
    out_len = torch.full((len(streams),), -1, dtype=torch.int64, device="cuda")
    status = torch.full((len(streams),), 0x7777, dtype=torch.int32, device="cuda")
    lens = [len(s) for s in streams]
    D.unsnap_ragged(dev(inp), in_off, lens, out, out_off, caps, out_len, status, D.snap_scratch(lens, caps))
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_off, out_len.cpu().tolist(), status.cpu().tolist()


@pytest.fixture(scope="module")
def reference():
    """The object set with the host's and the oracle's streams, and the
    condition that a weak input set cannot hide a failure."""
    from oracle import oracle as O
    objs = SD.objects()
    host = [host_snap(b) for _, b in objs]
    orc = [O.c_snap_compress(b) for _, b in objs]
    kinds = {name: SD.kinds(s) for (name, _), s in zip(objs, orc)}
    full = [f"mix40_{n}" for n in (4096, 4097, 16384, 16385, 65535, 65536, 200000)]
    assert all("raw" not in kinds[n] for n in full)                      # L = 40: compressed chunks only
    m40 = set().union(*(kinds[n] for n in full))
    assert {"compressed", "copy1", "copy2", "len60", "len64", "far", "overlap", "lit1", "lit2"} <= m40
    across = [k for n, k in kinds.items() if n.startswith(("mix300", "mix400"))]
    assert any({"raw", "compressed"} <= k for k in across) and any(k == {"raw"} for k in across)
    assert any("lit3" in k for k in across)
    assert {"raw"} == kinds["random65537"] and "compressed" in kinds["zeros200000"]
    return objs, host, orc


@pytest.fixture(scope="module")
def compressed(gpu, reference):
    objs, host, orc = reference
    return run_snap([b for _, b in objs])


def test_raw_compress_equals_the_host_and_the_oracle_and_touches_nothing_else(gpu, reference, compressed):
    objs, host, orc = reference
    image, out_off, out_len, want = compressed
    assert len(objs) >= 50 and {o % 16 for o in out_off} == set(range(16))
    for o, s in enumerate(host):
        assert s == orc[o], objs[o][0]
        want[out_off[o]:out_off[o] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    assert out_len == [len(s) for s in host]
    bad = np.flatnonzero(image != want)
    assert bad.size == 0, (bad[:8].tolist(), [n for (n, _), off in zip(objs, out_off) if off <= bad[0]][-1])


def test_raw_compress_of_one_object_whose_worst_case_is_16_mib(gpu):
    n = (16 << 20) - 10 - 8 * 256 - 97
    data = SD.mix(n, 40, 7)
    image, out_off, out_len, want = run_snap([data])
    s = host_snap(data)
    want[out_off[0]:out_off[0] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    assert out_len == [len(s)] and np.array_equal(image, want)
    out, off, olen, status = run_unsnap([s], [n])
    assert status == [OK] and olen == [n] and bytes(out[:n]) == data


def handbuilt():
    """(stream, content) of valid streams no compressor here writes."""
    lit = b"abcdefgh"
    out = []
    body = SD.varint(16) + SD.literal(lit) + SD.copy4(8, 8)
    out.append((SD.STREAM_ID + SD.data_chunk(lit * 2, body), lit * 2))                       # a copy-4 tag
    for hb in (4, 5):                                                                       # long literal headers
        body = SD.varint(300) + SD.literal(bytes(range(250)) + bytes(50), hb)
        out.append((SD.STREAM_ID + SD.data_chunk(bytes(range(250)) + bytes(50), body), bytes(range(250)) + bytes(50)))
    for off in range(1, 8):                                                                 # overlapping copies
        seed = bytes(range(65, 72))
        content = seed + SD.expand(seed[-off:], 64) + SD.expand((seed + SD.expand(seed[-off:], 64))[-off:], 9)
        body = SD.varint(len(content)) + SD.literal(seed) + SD.copy2(off, 64) + SD.copy1(off, 9)
        out.append((SD.STREAM_ID + SD.data_chunk(content, body), content))
    a, b = b"first block " * 10, b"second block" * 7
    out.append((SD.STREAM_ID + SD.data_chunk(a) + SD.chunk(0x80, b"padding") + SD.data_chunk(b) +
                SD.chunk(0xFE, bytes(100)), a + b))                                         # skippable chunks
    out.append((SD.STREAM_ID + SD.data_chunk(a) + SD.STREAM_ID + SD.data_chunk(b), a + b))  # a second identifier
    out.append((SD.STREAM_ID, b""))                                                         # identifier only
    out.append((b"", b""))                                                                  # empty
    return out


def test_raw_decompress_of_device_host_oracle_and_handbuilt_streams(gpu, reference, compressed):
    from oracle import host_oracle as H
    from oracle import oracle as O
    objs, host, orc = reference
    image, c_off, c_len, _ = compressed
    streams, contents = [], []
    for o, (name, b) in enumerate(objs):
        streams.append(bytes(image[c_off[o]:c_off[o] + c_len[o]]))       # the device's
        contents.append(b)
        if o % 3 == 0:
            streams.append(orc[o])                                       # the C oracle's
            contents.append(b)
        if len(b) <= 20000 and o % 2 == 0:
            streams.append(H.snap_compress(b))                           # the Python oracle's
            contents.append(b)
    for s, c in handbuilt():
        streams.append(s)
        contents.append(c)
    caps = [len(c) + (o % 3) * 7 for o, c in enumerate(contents)]        # exact, and with room to spare
    out, off, olen, status = run_unsnap(streams, caps)
    want = np.full(out.size, 0x5A, dtype=np.uint8)
    for o, (s, c) in enumerate(zip(streams, contents)):
        st, n, got = host_unsnap(s, caps[o])
        assert (st, n, got) == (OK, len(c), c), o
        assert O.c_snap_decompress(s, caps[o]) == c, o
        want[off[o]:off[o] + len(c)] = np.frombuffer(c, dtype=np.uint8)
    assert status == [OK] * len(streams) and olen == [len(c) for c in contents]
    assert np.array_equal(out, want)


def corrupt_cases(reference):
    """(stream, capacity, kind, needed length): kind 'framing' and 'small'
    leave the range untouched, 'block' leaves zeros over the needed length,
    'many' is a valid stream with more data chunks than slots."""
    objs, host, _ = reference
    by = {name: (b, s) for (name, b), s in zip(objs, host)}
    rnd, rs = by["random65537"]        # two raw chunks
    mx, ms = by["mix40_65536"]         # one compressed chunk
    small, ss = by["mix40_4096"]

    def flip(s, at, bit=0x10):
        b = bytearray(s)
        b[at] ^= bit
        return bytes(b)

    def one(body, content_len, crc_of=b""):
        return SD.STREAM_ID + SD.data_chunk(crc_of, body), content_len

    cases = [
        (flip(ms, 10 + 4 + 2), len(mx), "block", len(mx)),                       # a flipped CRC bit
        (flip(rs, 10 + 8 + 3000), len(rnd), "block", len(rnd)),                  # a body byte of a raw chunk
        (flip(ms, 10 + 8 + 5000), len(mx), "block", len(mx)),                    # ... of a compressed chunk
        (flip(ss, 10, 0x02), len(small), "framing", 0),                          # chunk type 0x02
        (ss[10:], len(small), "framing", 0),                                     # no identifier
        (ss[:-5], len(small), "framing", 0),                                     # a chunk length past the end
        (SD.STREAM_ID + SD.chunk(0x01, b"abc"), 16, "framing", 0),               # chunk length 3
        (SD.STREAM_ID + SD.data_chunk(b"", SD.varint(65537) + b"\x00"), 70000, "framing", 0),   # varint length 65537
        (SD.STREAM_ID + SD.chunk(0x01, bytes(4) + bytes(65537)), 70000, "framing", 0),         # a raw chunk of 65537
        (ss, len(small) - 1, "small", len(small)),                               # capacity one byte short
    ]
    lit = bytes(range(1, 5))
    for body, n in (
            (SD.varint(8) + SD.literal(lit) + SD.copy2(0, 4), 8),                # offset 0
            (SD.varint(8) + SD.literal(lit) + SD.copy2(5, 4), 8),                # offset > written
            (SD.varint(8) + bytes([7 << 2]) + lit, 8),                           # a literal running past the body
            (SD.varint(6) + SD.literal(lit) + SD.copy2(4, 4), 6),                # a copy running past the block
            (SD.varint(9) + SD.literal(lit), 9)):                                # a block ending short of its varint
        s, need = one(body, n)
        cases.append((s, n + 3, "block", need))
    many = SD.STREAM_ID + b"".join(SD.data_chunk(bytes([65 + i]) * 5) for i in range(4))
    cases.append((many, 100, "many", 20))                                        # 4 data chunks, 2 slots
    return cases


def test_corrupt_streams_fail_alone_with_the_hosts_status(gpu, reference):
    objs, host, _ = reference
    cases = corrupt_cases(reference)
    good_c, good_s = objs[SD.LENGTHS.index(4097)][1], host[SD.LENGTHS.index(4097)]
    streams, caps = [good_s], [len(good_c)]
    for s, cap, _, _ in cases:
        streams += [s, good_s]
        caps += [cap, len(good_c)]
    out, off, olen, status = run_unsnap(streams, caps)
    want = np.full(out.size, 0x5A, dtype=np.uint8)
    for o in range(0, len(streams), 2):                                           # the healthy neighbours
        want[off[o]:off[o] + len(good_c)] = np.frombuffer(good_c, dtype=np.uint8)
        assert status[o] == OK and olen[o] == len(good_c), o
    for i, (s, cap, kind, need) in enumerate(cases):
        o = 2 * i + 1
        st, n, _ = host_unsnap(s, cap)
        if kind == "many":
            assert st == OK and n == need and status[o] == MANY and olen[o] == 0, i
            continue
        assert status[o] == st, (i, kind, status[o], st)
        assert st == (TOO_SMALL if kind == "small" else SNAP), (i, kind, st)
        assert olen[o] == (n if kind == "small" else 0), (i, kind)
        if kind == "small":
            assert n == need
        if kind == "block":
            assert need <= cap
            want[off[o]:off[o] + need] = 0
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, bad[:8].tolist()


# ---- formats 14, 15, 10, 7 and 6 in one call: against orc_encode_full (all in
# C, with the injected values) and against chip_encode with the same injection

class Batch:
    def __init__(self, fmt, datas, seed):
        from carbonado_amd import device as D
        from oracle import oracle as O
        self.fmt, self.pt, self.count = fmt, datas, len(datas)
        self.lens = [len(d) for d in datas]
        self.pub = O.c_public_key(SECRET) if fmt & 1 else None
        rng = np.random.default_rng(seed)
        self.inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(),
                        rng.integers(0, 256, 16, dtype=np.uint8).tobytes()) for _ in datas] if fmt & 1 else None
        self.in_off, pos = [], 0
        for n in self.lens:
            self.in_off.append(pos)
            pos += up16(n) + 16
        self.in_size = pos + 16
        self.out_off, self.cap, self.total = D.snap_encode_layout(fmt, self.lens, 256, 56 if fmt & 4 else 0)

    def plain_image(self, fill, skip=(), zero=()):
        img = np.full(self.in_size, fill, dtype=np.uint8)
        for o, d in enumerate(self.pt):
            if o in zero:
                img[self.in_off[o]:self.in_off[o] + len(d)] = 0
            elif o not in skip:
                img[self.in_off[o]:self.in_off[o] + len(d)] = np.frombuffer(d, dtype=np.uint8)
        return img

    def oracle(self, o):
        from oracle import oracle as O
        if self.fmt & 1:
            return O.c_encode_full(self.pt[o], self.fmt, self.pub, *self.inject[o])
        return O.c_encode_full(self.pt[o], self.fmt)

    def encode(self):
        from carbonado_amd import device as D
        out = torch.full((self.total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        hashes = torch.full((self.count, 32), 0xEE, dtype=torch.uint8, device="cuda")
        olen, info = D.encode_ragged_snap(self.fmt, dev(self.plain_image(0x11)), self.in_off, self.lens, out,
                                          self.out_off, hashes, D.snap_ragged_scratch(self.fmt, self.lens),
                                          pubkey=self.pub, inject=self.inject)
        torch.cuda.synchronize()
        return out, hashes, olen, info

    def decode(self, out, hashes, olen, pads, secret=SECRET):
        from carbonado_amd import device as D
        back = torch.full((self.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.full((self.count,), 0x7777, dtype=torch.int32, device="cuda")
        got = torch.full((self.count,), -1, dtype=torch.int64, device="cuda")
        D.decode_ragged_snap(self.fmt, out, self.out_off, olen, hashes, pads, back, self.in_off, self.lens, got, status,
                             D.snap_ragged_scratch(self.fmt, olen, self.lens),
                             secret_key=secret if self.fmt & 1 else None)
        torch.cuda.synchronize()
        return back.cpu().numpy(), status.cpu().tolist(), got.cpu().tolist()


def _same_info(got, want: dict):
    for f, w in want.items():
        g = getattr(got, f)
        if isinstance(w, float) and math.isfinite(w):
            assert abs(g - w) <= 1e-6 * max(1.0, abs(w)), (f, g, w)
        else:  # integers; nan and inf for an empty input (0 / 0, x / 0), as the reference's f32 division gives
            assert g == w or (math.isnan(g) and math.isnan(w)), (f, g, w)


@pytest.mark.parametrize("fmt", [14, 15, 10, 7, 6])
def test_one_call_encode_equals_the_oracle_and_chip_encode_and_round_trips(gpu, reference, fmt):
    import carbonado_amd as ca
    objs = [b for i, (_, b) in enumerate(reference[0]) if i % 4 != 3]
    assert len(objs) >= 38 and 0 in [len(b) for b in objs]
    s = Batch(fmt, objs, seed=60 + fmt)
    out, hashes, olen, info = s.encode()
    image, hh = out.cpu().numpy(), hashes.cpu().numpy()
    want = np.full(image.size, 0xA5, dtype=np.uint8)
    for o in range(s.count):
        enc, h, winfo = s.oracle(o)
        assert olen[o] == len(enc) <= s.cap[o], o
        want[s.out_off[o]:s.out_off[o] + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
        assert bytes(hh[o]) == (h if fmt & 4 else bytes(32)), o
        _same_info(info[o], winfo)
        if o % 6 == 0:
            kw = dict(ephemeral_sk=s.inject[o][0], nonce=s.inject[o][1]) if fmt & 1 else {}
            cenc, ch, cinfo = ca.encode(s.pub or b"", s.pt[o], fmt, **kw)
            assert cenc == enc and ch == h
            _same_info(info[o], {f: getattr(cinfo, f) for f in winfo})
    bad = np.flatnonzero(image != want)                        # the streams, and nothing past out_len in the rows
    assert bad.size == 0, bad[:8].tolist()
    pads = [i.padding_len for i in info]
    for streams in (out, dev(want)):                           # the device's streams and the oracle's
        back, status, got = s.decode(streams, hashes, olen, pads)
        assert status == [OK] * s.count and got == s.lens
        assert np.array_equal(back, s.plain_image(0x5A))


@pytest.mark.parametrize("fmt", [14, 15])
def test_damage_keeps_the_earlier_stage_status_and_a_bad_frame_gives_16_alone(gpu, fmt):
    from carbonado_amd import device as D
    from oracle import oracle as O
    datas = [SD.mix(5000, 40, 1), b"", SD.mix(70001, 40, 2), SD.mix(1024, 40, 3), SD.mix(20000, 40, 4),
             SD.mix(300, 40, 5), SD.mix(9000, 40, 6)]
    s = Batch(fmt, datas, seed=77)
    out, hashes, olen, info = s.encode()
    pads = [i.padding_len for i in info]
    out[s.out_off[2] + olen[2] // 2] ^= 0x20                 # a damaged stream byte: bao's status, nothing decompressed

    def reencode(o, stage: bytes):
        """Object o's stream again at level 12 over other bytes of the same length (every hash in it is right)."""
        h = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
        ln, _ = D.encode_ragged(12, dev(np.frombuffer(stage, dtype=np.uint8)), [0], [len(stage)], out, [s.out_off[o]], h,
                                D.ragged_scratch(12, [len(stage)]))
        assert ln == [olen[o]]
        hashes[o] = h[0]

    def stage_of(o, frame: bytes, forge=None):
        if not fmt & 1:
            return frame
        env = bytearray(O.c_ecies_encrypt(s.pub, frame, *s.inject[o]))
        if forge is not None:
            env[97 + forge] ^= 0x01
        return bytes(env)

    frame4 = bytearray(host_snap(datas[4]))
    frame4[10 + 4 + 1] ^= 0x40                               # a CRC bit of the first chunk: a corrupt frame
    reencode(4, stage_of(4, bytes(frame4)))
    want_status = [OK, OK, BAO, OK, SNAP, OK, OK]
    skip, zero = {2}, {4}
    if fmt & 1:                                              # a stream re-encoded over a forged envelope
        reencode(6, stage_of(6, host_snap(datas[6]), forge=100))
        want_status[6] = ECIES
        skip.add(6)
    back, status, got = s.decode(out, hashes, olen, pads)
    assert status == want_status
    assert got == [n if st == OK else 0 for n, st in zip(s.lens, want_status)]
    assert np.array_equal(back, s.plain_image(0x5A, skip=skip, zero=zero))


def test_level_14_streams_are_level_12_streams_to_the_read_and_audit_calls(gpu):
    """read_ranges and verify_slices take the streams of encode_ragged_snap at
    14 as the level-12 streams (of the frame streams) they are."""
    from carbonado_amd import device as D
    rng = np.random.default_rng(5)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5000, 70001)] + [SD.mix(120000, 40, 9)]
    frames = [host_snap(d) for d in datas]
    s = Batch(14, datas, seed=47)
    out, hashes, olen, info = s.encode()
    pads, cls = [i.padding_len for i in info], [i.chunk_len for i in info]
    rs, start = [0, 1, 2, 1], [0, 97, 19000, 65000]
    length = [300, 4096, len(frames[2]) - 19000, len(frames[1]) - 65000]   # two end with their frame stream
    coff, clen, total, nseg = D.read_layout(cls, pads, rs, start, length)
    content = torch.full((total + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), 0x7777, dtype=torch.int32, device="cuda")
    used = torch.zeros(4, dtype=torch.int32, device="cuda")
    got = D.read_ranges(out, s.out_off, olen, hashes, pads, cls, rs, start, length, content, coff, status, used,
                        D.read_scratch(4, nseg))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 4 and got == clen == length
    host = content.cpu().numpy()
    for r in range(4):
        assert bytes(host[coff[r]:coff[r] + length[r]]) == frames[rs[r]][start[r]:start[r] + length[r]], r
    rs, idx, cnt = [0, 1, 2], [0, 0, 0], [1, 1, 1]
    _, _, coff, clen, _, ct = D.slice_layout([8 * c for c in cls], idx, cnt)
    content = torch.full((ct + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((3,), 0x7777, dtype=torch.int32, device="cuda")
    got = D.verify_slices(out, s.out_off, olen, hashes, rs, idx, cnt, content, coff, status, D.audit_scratch(3, 3))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 3 and got == [1024] * 3
    host = content.cpu().numpy()
    for r in range(3):
        assert min(cls) >= 1024 and bytes(host[coff[r]:coff[r] + 1024]) == frames[r][:1024], r
