"""Plaintext ranged reads of level-13 streams (include/carbonado_hip_cread.h).
The keystream layer is compared with EVP AES-256-GCM (16-byte IV) called
through ctypes on the libcrypto the library already links; the reads with
slices of the test's own plaintexts, encoded by encode_ragged_ecies with
injected ephemeral secrets and nonces.  Every comparison is of whole buffers
over a canary fill, so the bytes outside the ranges are checked too."""
import functools

import numpy as np
import pytest
import torch

from evp_gcm import evp_seal, j0_of  # tests/evp_gcm.py (tests/ is on sys.path under pytest)
from read_world import PlainStreams, dev, up16

pytestmark = pytest.mark.gpu

ECIES, VOUCHED = 17, 1
UNIT_SPAN = 127 * 16          # bytes of one wave's work item (cread_device.hpp: SPAN_UNITS * 16)
EDGES = [0, 1, 15, 16, 17, 31, 32, 33]
SECRET = bytes(range(1, 33))
WRAP_KEY = bytes.fromhex("c675bea6d150367b0fa6dbcb7e142508528234103f6d178e38a1ab8736270c09")
WRAP_IV = bytes.fromhex("5436aa0234896411575d56bbd2095dc7")


# ---- the keystream over ranges ------------------------------------------------------
class Items:
    """Items (key, pos, n) over messages sealed by EVP: the buffer holds the
    ciphertext slices at 16-B aligned offsets with canary gaps."""

    def __init__(self, keys, ivs, pts, items, fill=0xC5):
        self.keys, self.ivs = b"".join(keys), b"".join(ivs)
        self.ct = [evp_seal(k, v, p)[0] for k, v, p in zip(keys, ivs, pts)]
        self.pt = pts
        self.key = [k for k, _, _ in items]
        self.pos = [p for _, p, _ in items]
        self.n = [n for _, _, n in items]
        self.off, at = [], 0
        for n in self.n:
            self.off.append(at)
            at += up16(n) + 16
        self.size, self.fill = at + 16, fill

    def image(self, src, only=None):
        """The buffer with slices of src (self.ct or self.pt); `only`: items taken from self.pt, the others from self.ct."""
        img = np.full(self.size, self.fill, dtype=np.uint8)
        for i, (k, p, n, o) in enumerate(zip(self.key, self.pos, self.n, self.off)):
            s = src if only is None else (self.pt if only[i] else self.ct)
            img[o:o + n] = np.frombuffer(s[k][p:p + n], dtype=np.uint8)
        return img

    def run(self, buf, gate=None, scratch=None):
        from carbonado_amd import device as D
        scratch = scratch if scratch is not None else D.ctr_scratch(len(self.keys) // 32, len(self.n))
        D.ctr_ranges(self.keys, self.ivs, self.key, self.pos, self.n, buf, self.off, scratch, gate=gate)
        torch.cuda.synchronize()
        return buf.cpu().numpy()


def _raw_items():
    rng = np.random.default_rng(5)
    lens = [100, 20000, 70001]
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in lens]
    ivs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in lens]
    pts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    items = [(1, 48 * sh + sh, n) for sh in range(16) for n in EDGES]                      # every pos % 16 x the edges
    items += [(2, 1000 + sh, UNIT_SPAN + d) for sh in (0, 7, 15) for d in (-1, 0, 1)]     # around a span's edge
    items += [(2, 333, 2 * UNIT_SPAN + 1)]
    items += [(1, p, 100) for p in (8191, 8192, 8193)]
    items += [(0, 0, 100), (1, 5, 0), (2, 0, 0), (2, 70001 - 5000, 5000), (0, 99, 1)]       # whole, empty, to the last byte
    return Items(keys, ivs, pts, items)


def test_keystream_over_ranges_against_evp(gpu):
    from carbonado_amd import device as D
    it = _raw_items()
    assert 140 <= len(it.n) <= 160
    nkeys, nitems = 3, len(it.n)
    scratch = D.ctr_scratch(nkeys, nitems)
    scratch.fill_(0xFF)
    buf = dev(it.image(it.ct))
    got = it.run(buf, scratch=scratch)
    assert np.array_equal(got, it.image(it.pt))
    # the key region ([keys, end): behind the 40-byte item records) is zero afterwards
    assert scratch.numel() == up16(40 * nitems) + (48 + 512) * nkeys
    assert not scratch.cpu().numpy()[up16(40 * nitems):].any()
    # applied twice it is the identity
    assert np.array_equal(it.run(buf), it.image(it.ct))
    # a gate: the items whose word is not zero stay as they were
    gate = np.zeros(nitems, dtype=np.int32)
    gate[::3] = 7
    gate[5::11] = -1
    got = it.run(buf, gate=torch.from_numpy(gate).cuda())
    assert np.array_equal(got, it.image(None, only=(gate == 0)))


def test_counter_wraps_in_the_low_word_only(gpu):
    n = 1 << 20
    j0 = j0_of(WRAP_KEY, WRAP_IV)
    istar = (1 << 32) - 1 - (j0 & 0xFFFFFFFF)
    assert istar == 0x85d9 and 16 * (istar + 2) < n, "the committed pair must wrap inside the message"
    pt = np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes()
    start = 16 * istar - 41
    assert start % 16 % 2 == 1
    it = Items([WRAP_KEY], [WRAP_IV], [pt], [(0, start, 100), (0, 16 * (istar + 1), 100), (0, 16 * istar + 3, 5000)])
    assert np.array_equal(it.run(dev(it.image(it.ct))), it.image(it.pt))


# ---- reads of level-13 streams ---------------------------------------------------------
SIZES = [0, 1, 926, 927, 928, 5000, 70001, 300001]
BIG = 6  # the stream the damage cases use


class Streams(PlainStreams):
    def __init__(self):
        from carbonado_amd import device as D
        from oracle import oracle as O
        rng = np.random.default_rng(61)
        self.count = len(SIZES)
        self.pub = O.c_public_key(SECRET)
        self.pt = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in SIZES]
        self.inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
                       for _ in SIZES]
        self.env = [O.c_ecies_encrypt(self.pub, p, sk, nonce) for p, (sk, nonce) in zip(self.pt, self.inject)]
        in_off, plain = self.place_plain(SIZES)
        self.off, _, total = D.ragged_layout(12, [n + 97 for n in SIZES], 256)
        self.make_outputs(total, self.count)
        self.olen, info = D.encode_ragged_ecies(13, self.pub, dev(plain), in_off, SIZES, self.out, self.off, self.hashes,
                                                D.ecies_ragged_scratch(13, SIZES), inject=self.inject)
        torch.cuda.synchronize()
        self.pads, self.cls = [i.padding_len for i in info], [i.chunk_len for i in info]
        self.keys = self.ivs = None
        # requests in plaintext bytes
        self.reqs = []
        for s, P in enumerate(SIZES):
            C = self.cls[s]
            rq = [(0, P), (0, 1), (max(P - 1, 0), 1), (P + 5, 10), (min(3, P), 0), (max(P - 10, 0), 100),
                  (1024 - 97 - 10, 20)]
            rq += [(k * C - 97 - 20, 40) for k in (1, 2, 3) if k * C - 97 + 20 <= P]
            rq += [(17 * sh, 33) for sh in range(16)]
            self.reqs += [(s, a, n) for a, n in rq]

    def damaged(self, s, chunks, byte=500):
        """A copy of the streams with one byte flipped in each of stream s's chunks given as (shard, chunk)."""
        spc = self.cls[s] // 1024
        return self.flipped(self.chunk_pos(s, shard * spc + c, byte) for shard, c in chunks)

    def stream_keys(self, out=None, secret=SECRET):
        from carbonado_amd import device as D
        return D.stream_keys(secret, self.out if out is None else out, self.off, self.olen, self.hashes, self.pads,
                             self.cls, D.stream_keys_scratch(self.count))

    def read(self, reqs, keys, ivs, key_status=None, out=None, flags=0):
        """(content image, status, used, vouch, content_off, content_len) of read_plain_ranges."""
        from carbonado_amd import device as D
        rs, start, length = [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]
        coff, clen, total, nseg = D.plain_read_layout(self.cls, self.pads, rs, start, length)
        content = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        st, used, vouch = (torch.full((len(reqs),), 0x7777, dtype=torch.int32, device="cuda") for _ in range(3))
        got = D.read_plain_ranges(keys, ivs, key_status, self.out if out is None else out, self.off, self.olen,
                                  self.hashes, self.pads, self.cls, rs, start, length, content, coff, st, used, vouch,
                                  D.plain_read_scratch(len(reqs), nseg, self.count), flags=flags)
        torch.cuda.synchronize()
        assert got == clen
        return content.cpu().numpy(), st.cpu().tolist(), used.cpu().tolist(), vouch.cpu().tolist(), coff, clen


@functools.lru_cache(maxsize=None)
def streams() -> Streams:
    s = Streams()
    s.keys, s.ivs, status = s.stream_keys()
    assert status.tolist() == [0] * s.count
    return s


def test_stream_keys_are_those_the_envelopes_imply(gpu):
    s = streams()
    for o in range(s.count):
        assert bytes(s.ivs[o]) == s.env[o][65:81] == s.inject[o][1], o
        ct, tag = evp_seal(bytes(s.keys[o]), bytes(s.ivs[o]), s.pt[o])   # the key that seals this plaintext to this envelope
        assert ct == s.env[o][97:] and tag == s.env[o][81:97], o


def test_plaintext_ranges_of_intact_streams(gpu):
    s = streams()
    content, status, used, vouch, coff, clen = s.read(s.reqs, s.keys, s.ivs)
    assert status == [0] * len(s.reqs) and vouch == [0] * len(s.reqs)
    assert clen == [len(s.pt[o][a:a + n]) for o, a, n in s.reqs]
    assert np.array_equal(content, s.want(s.reqs, coff, content.size))
    starts = {a % 16 for o, a, n in s.reqs if o == BIG and n}
    assert starts == set(range(16))


def test_the_read_is_the_vouched_read_and_the_keystream(gpu):
    from carbonado_amd import device as D
    s = streams()
    content, status, used, vouch, coff, clen = s.read(s.reqs, s.keys, s.ivs)
    rs, start, length = [r[0] for r in s.reqs], [r[1] + 97 for r in s.reqs], [r[2] for r in s.reqs]
    voff, vlen, total, nseg = D.read_layout(s.cls, s.pads, rs, start, length)
    assert (voff, vlen) == (coff, clen)
    buf = torch.full((content.size,), 0xA5, dtype=torch.uint8, device="cuda")
    st, us, vo = (torch.full((len(rs),), 0x7777, dtype=torch.int32, device="cuda") for _ in range(3))
    D.read_ranges_vouched(s.out, s.off, s.olen, s.hashes, s.pads, s.cls, rs, start, length, buf, voff, st, us, vo,
                          D.vread_scratch(len(rs), nseg))
    D.ctr_ranges(s.keys, s.ivs, rs, [r[1] for r in s.reqs], vlen, buf, voff, D.ctr_scratch(s.count, len(rs)))
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), content)
    assert (st.cpu().tolist(), us.cpu().tolist(), vo.cpu().tolist()) == (status, used, vouch)


def _big_requests(s):
    C = s.cls[BIG]
    window = (BIG, C - 97 + 1024 + 100, 300)     # columns 1124 .. 1424 of primary 1: its chunk 1
    return [window, (BIG, 0, 1), (BIG, 3 * C, 500), (5, 100, 4000), (BIG, SIZES[BIG] - 1, 1)]


def test_a_damaged_window_is_rebuilt_and_vouched_for_or_fails_alone(gpu):
    s = streams()
    reqs = _big_requests(s)
    content, status, used, vouch, coff, _ = s.read(reqs, s.keys, s.ivs, out=s.damaged(BIG, [(1, 1)]))
    assert status == [0] * 5 and vouch == [VOUCHED, 0, 0, 0, 0]
    assert bin(used[0]).count("1") == 4 and not used[0] & 2 and used[1] == 1
    assert np.array_equal(content, s.want(reqs, coff, content.size))
    # the same window damaged in five shards: status 7 and zeros, the stream's other requests still served
    bad = s.damaged(BIG, [(i, 1) for i in (1, 2, 3, 4, 5)])
    content, status, used, vouch, coff, _ = s.read(reqs, s.keys, s.ivs, out=bad)
    assert status == [7, 0, 0, 0, 0] and used[0] == 0 and vouch[0] == 0
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0}))


def test_a_damaged_header_is_rebuilt_for_the_key_or_fails_its_stream(gpu):
    s = streams()
    reqs = _big_requests(s)
    bad = s.damaged(BIG, [(0, 0)], byte=30)          # inside the ephemeral key
    keys, ivs, status = s.stream_keys(out=bad)
    assert status.tolist() == [0] * s.count and np.array_equal(keys, s.keys) and np.array_equal(ivs, s.ivs)
    bad = s.damaged(BIG, [(i, 0) for i in range(5)], byte=30)
    keys, ivs, kstat = s.stream_keys(out=bad)
    assert kstat.tolist() == [7 if o == BIG else 0 for o in range(s.count)]
    assert not keys[BIG].any() and not ivs[BIG].any()
    assert np.array_equal(np.delete(keys, BIG, 0), np.delete(s.keys, BIG, 0))
    content, status, used, vouch, coff, _ = s.read(reqs, keys, ivs, key_status=kstat, out=bad)
    assert status == [7, 7, 7, 0, 7] and used[:3] + used[4:] == [0] * 4 and vouch == [0] * 5
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0, 1, 2, 4}))
    # a key status of every kind, and a request without bytes on a stream without a key
    kstat = np.array([5, 17, 0, 0, 0, 0, 7, 0], dtype=np.uint32)
    reqs = [(0, 0, 5), (1, 0, 1), (1, 0, 0), (2, 10, 50), (BIG, 100, 3000)]
    content, status, used, vouch, coff, _ = s.read(reqs, s.keys, s.ivs, key_status=kstat)
    assert status == [5, 17, 17, 0, 7] and used[:3] + used[4:] == [0] * 4 and vouch == [0] * 5
    assert np.array_equal(content, s.want(reqs, coff, content.size, zero={0, 1, 2, 4}))


def test_envelope_faults_and_the_documented_limit(gpu):
    from carbonado_amd import device as D
    s = streams()
    # level-12 streams over a forged envelope (every hash in it is right) and over an object too short to be one
    env = bytearray(s.env[5])
    env[0] = 0x05
    objs = [bytes(env), bytes(range(50))]
    sizes = [len(o) for o in objs]
    inp = np.zeros(up16(sizes[0]) + 64, dtype=np.uint8)
    inp[:sizes[0]] = np.frombuffer(objs[0], dtype=np.uint8)
    inp[up16(sizes[0]):up16(sizes[0]) + 50] = np.frombuffer(objs[1], dtype=np.uint8)
    off, _, total = D.ragged_layout(12, sizes, 256)
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    hashes = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    olen, info = D.encode_ragged(12, dev(inp), [0, up16(sizes[0])], sizes, out, off, hashes, D.ragged_scratch(12, sizes))
    keys, ivs, kstat = D.stream_keys(SECRET, out, off, olen, hashes, [i.padding_len for i in info],
                                     [i.chunk_len for i in info], D.stream_keys_scratch(2))
    assert kstat.tolist() == [ECIES, ECIES] and not keys.any() and not ivs.any()
    # a wrong secret key: status 0 and bytes that are not the plaintext (nothing in a range proves the key)
    keys, ivs, kstat = s.stream_keys(secret=bytes(range(3, 35)))
    assert kstat.tolist() == [0] * s.count and np.array_equal(ivs, s.ivs) and not np.array_equal(keys, s.keys)
    reqs = [(5, 100, 4000), (BIG, 0, 1000)]
    content, status, used, vouch, coff, clen = s.read(reqs, keys, ivs, key_status=kstat)
    assert status == [0, 0] and clen == [4000, 1000]
    want = s.want(reqs, coff, content.size)
    for r in range(2):
        assert not np.array_equal(content[coff[r]:coff[r] + clen[r]], want[coff[r]:coff[r] + clen[r]])
    live = np.ones(content.size, dtype=bool)
    for r in range(2):
        live[coff[r]:coff[r] + clen[r]] = False
    assert (content[live] == 0xA5).all()
