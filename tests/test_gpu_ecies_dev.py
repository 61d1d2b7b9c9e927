"""AES-256-GCM over device-resident messages (include/carbonado_hip_ecies.h)
against EVP AES-256-GCM with a 16-byte IV, called through ctypes on the
libcrypto the library already links: a reference that shares nothing with the
bitsliced AES and the table-free GHASH under test.  Every comparison is of
whole buffers, so the bytes between the output ranges (a canary fill) are
checked with the ranges themselves."""
import math

import numpy as np
import pytest
import torch

from evp_gcm import evp_seal, j0_of  # tests/evp_gcm.py (tests/ is on sys.path under pytest)
from read_world import dev, up16

pytestmark = pytest.mark.gpu

ECIES = 17
ITEM = 8192                   # bytes of one wave's item (gcm_device.hpp: SPAN * 16)
LEVEL2 = 64 * ITEM            # 64 items: one step of the second level
EDGES = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, ITEM - 1, ITEM, ITEM + 1,
         2 * ITEM - 1, 2 * ITEM, 2 * ITEM + 1, LEVEL2 - 1, LEVEL2, LEVEL2 + 1]


class Batch:
    """A ragged batch: plaintexts packed at 16-B aligned offsets, ciphertexts
    at the offsets given by `residues` (message o at residue residues[o % len]
    mod 16, a few bytes of gap in between), EVP's bytes for both."""

    def __init__(self, lens, seed, residues=tuple(range(16)), keys=None, ivs=None):
        rng = np.random.default_rng(seed)
        self.lens = list(lens)
        self.count = len(self.lens)
        self.keys = keys or rng.integers(0, 256, 32 * self.count, dtype=np.uint8).tobytes()
        self.ivs = ivs or rng.integers(0, 256, 16 * self.count, dtype=np.uint8).tobytes()
        self.pt = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in self.lens]
        self.in_off, self.out_off = [], []
        ip, op = 0, 0
        for o, n in enumerate(self.lens):
            self.in_off.append(ip)
            ip += up16(n) + 16 * (o % 3)
            op = up16(op) + 16 + residues[o % len(residues)]
            self.out_off.append(op)
            op += n
        self.in_size, self.out_size = ip + 16, up16(op) + 32
        self.ct, self.tags = [], []
        for o in range(self.count):
            c, t = evp_seal(self.keys[32 * o:32 * o + 32], self.ivs[16 * o:16 * o + 16], self.pt[o])
            self.ct.append(c)
            self.tags.append(t)

    def plain_image(self, fill: int, zero=()) -> np.ndarray:
        img = np.full(self.in_size, fill, dtype=np.uint8)
        for o, n in enumerate(self.lens):
            img[self.in_off[o]:self.in_off[o] + n] = 0 if o in zero else np.frombuffer(self.pt[o], dtype=np.uint8)
        return img

    def cipher_image(self, fill: int) -> np.ndarray:
        img = np.full(self.out_size, fill, dtype=np.uint8)
        for o, n in enumerate(self.lens):
            img[self.out_off[o]:self.out_off[o] + n] = np.frombuffer(self.ct[o], dtype=np.uint8)
        return img


def seal(b: Batch, fill=0xA5):
    from carbonado_amd import device as D
    inp = dev(b.plain_image(0x11))
    out = torch.full((b.out_size,), fill, dtype=torch.uint8, device="cuda")
    tags = torch.full((16 * b.count + 16,), fill, dtype=torch.uint8, device="cuda")
    scratch = D.gcm_scratch(b.lens)
    D.gcm_seal_ragged(b.keys, b.ivs, inp, b.in_off, b.lens, out, b.out_off, tags, scratch)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tags.cpu().numpy(), scratch


def open_(b: Batch, cipher: np.ndarray, tags: bytes, keys=None, dirty=None):
    from carbonado_amd import device as D
    inp = dev(cipher)
    out = dev(dirty) if dirty is not None else torch.full((b.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((b.count + 1,), 0x7777, dtype=torch.int32, device="cuda")
    scratch = D.gcm_scratch(b.lens)
    D.gcm_open_ragged(keys or b.keys, b.ivs, inp, b.out_off, b.lens, dev(np.frombuffer(tags, dtype=np.uint8)), out,
                      b.in_off, status, scratch)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy(), scratch


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(2026)
    lens = EDGES + [int(x) for x in rng.integers(0, 3000, 170)] + [(1 << 20) + 5, 4 << 20]
    return Batch(lens, seed=7)


def test_raw_seal_equals_evp_and_touches_nothing_else(gpu, mixed):
    out, tags, _ = seal(mixed)
    assert bytes(tags[:16 * mixed.count]) == b"".join(mixed.tags)
    assert bytes(tags[16 * mixed.count:]) == b"\xA5" * 16
    want = mixed.cipher_image(0xA5)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"first differing byte at {bad[:4]}"


def test_raw_open_returns_the_plaintext(gpu, mixed):
    out, status, _ = open_(mixed, mixed.cipher_image(0x3C), b"".join(mixed.tags) + bytes(16))
    assert (status[:mixed.count] == 0).all() and status[mixed.count] == 0x7777
    want = mixed.plain_image(0x5A)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"first differing byte at {bad[:4]}"


# A (key, IV) pair whose J0 ends in 0xffff7a26: a 1 MiB message (2^16 blocks)
# takes the counter's low word through 2^32.  Found once by a seeded search on
# the CPU (H from EVP AES-256-ECB of the zero block, GHASH in Python integers).
WRAP_KEY = bytes.fromhex("c675bea6d150367b0fa6dbcb7e142508528234103f6d178e38a1ab8736270c09")
WRAP_IV = bytes.fromhex("5436aa0234896411575d56bbd2095dc7")


def test_counter_wraps_in_the_low_word_only(gpu):
    n = 1 << 20
    j0 = j0_of(WRAP_KEY, WRAP_IV)
    assert j0 & 0xFFFFFFFF == 0xFFFF7A26 and (j0 & 0xFFFFFFFF) + n // 16 > 1 << 32, "the committed pair must wrap inside the message"
    b = Batch([n, 100], seed=3, residues=(1,), keys=WRAP_KEY + bytes(range(32)), ivs=WRAP_IV + bytes(range(16)))
    out, tags, _ = seal(b)
    assert bytes(tags[:32]) == b"".join(b.tags)
    assert np.array_equal(out, b.cipher_image(0xA5))
    back, status, _ = open_(b, out, bytes(tags[:32]))
    assert (status[:2] == 0).all() and np.array_equal(back, b.plain_image(0x5A))


@pytest.mark.parametrize("dirty_seed", [None, 5])
def test_forgeries_fail_alone_and_leave_zeros(gpu, dirty_seed):
    lens = [100, 0, 5000, 33, 20000, 16, 1, 3 * ITEM + 7, 0, 64, 1025, 17]
    b = Batch(lens, seed=11, residues=(1, 0, 7, 15))
    cipher = b.cipher_image(0x3C)
    tags = bytearray(b"".join(b.tags))
    keys = bytearray(b.keys)
    cipher[b.out_off[2] + 4321] ^= 0x01        # a ciphertext bit
    cipher[b.out_off[7] + 3 * ITEM + 6] ^= 0x80  # the last byte of a message of several items
    tags[16 * 4 + 15] ^= 0x01                  # a tag bit
    tags[16 * 8] ^= 0x40                       # the tag of an empty message
    keys[32 * 10 + 31] ^= 0x01                 # a wrong key
    failed = {2, 7, 4, 8, 10}
    dirty = None
    if dirty_seed is not None:
        dirty = np.random.default_rng(dirty_seed).integers(0, 256, b.in_size, dtype=np.uint8)
    out, status, _ = open_(b, cipher, bytes(tags), keys=bytes(keys), dirty=dirty)
    assert status[:b.count].tolist() == [ECIES if o in failed else 0 for o in range(b.count)]
    want = b.plain_image(0x5A, zero=failed)
    if dirty is not None:  # the bytes between the ranges keep what they held
        keep = np.ones(b.in_size, dtype=bool)
        for o, n in enumerate(lens):
            keep[b.in_off[o]:b.in_off[o] + n] = False
        want[keep] = dirty[keep]
    assert np.array_equal(out, want)


def test_key_region_of_the_scratch_is_zero_after_the_call(gpu):
    b = Batch([100, 0, 3 * ITEM + 1, 16], seed=13)
    for scratch in (seal(b)[2], open_(b, b.cipher_image(0), b"".join(b.tags))[2]):
        s = scratch.cpu().numpy()
        lo, hi = up16(48 * b.count) + 96 * b.count, s.size - up16(4 * b.count)  # behind the public table, before the verdict words
        assert hi - lo > b.count * (48 + 480 + 2 * 65 * 16)      # keys, round keys, powers of H
        assert not s[lo:hi].any()
        assert s[:lo].any()  # (the public table in front of it is not wiped)


def test_one_message_of_16_mib_less_an_envelope_header(gpu):
    """The ciphertext of the largest object an envelope holds, where an
    envelope puts it: 97 bytes into a 16-B aligned buffer, 2048 items."""
    b = Batch([(16 << 20) - 97], seed=17, residues=(1,))
    assert b.out_off[0] % 16 == 1
    out, tags, _ = seal(b)
    assert bytes(tags[:16]) == b.tags[0] and np.array_equal(out, b.cipher_image(0xA5))
    back, status, _ = open_(b, out, bytes(tags[:16]))
    assert status[0] == 0 and np.array_equal(back, b.plain_image(0x5A))


# ---- envelopes: encoding::ecies / decoding::ecies of resident objects against
# the C oracle's ecies (oracle/liboracle.so: orc_ecies_encrypt / orc_ecies_decrypt)

SECRET = bytes(range(1, 33))
ENV_LENS = [0, 1, 15, 16, 17, 33, 1000, 1024, ITEM - 97, ITEM - 96, ITEM, ITEM + 1, 20000, 100000]


class Envelopes:
    """Objects at 16-B aligned offsets, their envelopes at 16-B aligned offsets
    (the ciphertext then sits at 1 mod 16, as in the scratch of an encode) or
    at the residues given."""

    def __init__(self, lens, seed, residues=(0,)):
        from oracle import oracle as O
        rng = np.random.default_rng(seed)
        self.lens, self.count = list(lens), len(lens)
        self.pub = O.c_public_key(SECRET)
        self.pt = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in self.lens]
        self.inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
                       for _ in self.lens]
        self.env = [O.c_ecies_encrypt(self.pub, p, sk, nonce) for p, (sk, nonce) in zip(self.pt, self.inject)]
        self.in_off, self.env_off = [], []
        ip, ep = 0, 0
        for o, n in enumerate(self.lens):
            self.in_off.append(ip)
            ip += up16(n) + 16
            ep = up16(ep) + 16 + residues[o % len(residues)]
            self.env_off.append(ep)
            ep += n + 97
        self.in_size, self.env_size = ip + 16, up16(ep) + 32

    def plain_image(self, fill, zero=()):
        img = np.full(self.in_size, fill, dtype=np.uint8)
        for o, n in enumerate(self.lens):
            img[self.in_off[o]:self.in_off[o] + n] = 0 if o in zero else np.frombuffer(self.pt[o], dtype=np.uint8)
        return img

    def env_image(self, fill, envs=None):
        img = np.full(self.env_size, fill, dtype=np.uint8)
        for o, e in enumerate(envs or self.env):
            img[self.env_off[o]:self.env_off[o] + len(e)] = np.frombuffer(e, dtype=np.uint8)
        return img


def env_seal(e: Envelopes, inject=True):
    from carbonado_amd import device as D
    out = torch.full((e.env_size,), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = D.gcm_scratch(e.lens)
    D.ecies_seal_ragged(e.pub, dev(e.plain_image(0x11)), e.in_off, e.lens, out, e.env_off, scratch,
                        inject=e.inject if inject else None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), scratch


def env_open(e: Envelopes, image: np.ndarray, in_len=None, secret=SECRET):
    from carbonado_amd import device as D
    in_len = in_len or [n + 97 for n in e.lens]
    out = torch.full((e.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((e.count,), 0x7777, dtype=torch.int32, device="cuda")
    scratch = D.gcm_scratch([max(0, n - 97) for n in in_len])
    olen = D.ecies_open_ragged(secret, dev(image), e.env_off, in_len, out, e.in_off, status, scratch)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy().tolist(), olen


@pytest.fixture(scope="module")
def envelopes():
    return Envelopes(ENV_LENS, seed=23)


@pytest.mark.parametrize("residues", [(0,), (3, 8, 15, 0)])
def test_injected_seal_equals_the_oracles_envelopes(gpu, residues):
    e = Envelopes(ENV_LENS, seed=23, residues=residues)
    out, scratch = env_seal(e)
    assert np.array_equal(out, e.env_image(0xA5))
    s = scratch.cpu().numpy()
    assert not s[up16(48 * e.count) + 96 * e.count:s.size - up16(4 * e.count)].any()  # the key region


def test_open_of_device_and_oracle_envelopes(gpu, envelopes):
    from oracle import oracle as O
    e = envelopes
    sealed, _ = env_seal(e)
    for image in (sealed, e.env_image(0x3C)):
        out, status, olen = env_open(e, image)
        assert status == [0] * e.count and olen == e.lens
        assert np.array_equal(out, e.plain_image(0x5A))
    for o in (1, 6, 12):  # and the oracle opens what the device sealed
        got = bytes(sealed[e.env_off[o]:e.env_off[o] + e.lens[o] + 97])
        assert O.c_ecies_decrypt(SECRET, got) == e.pt[o]


def test_short_envelope_and_bad_ephemeral_key_fail_alone(gpu, envelopes):
    e = envelopes
    image = e.env_image(0x3C)
    in_len = [n + 97 for n in e.lens]
    in_len[2] = 96                                   # shorter than an envelope's overhead
    image[e.env_off[5] + 1:e.env_off[5] + 65] = 0xFF  # x = y = 2^256 - 1: not a point (not even a field element)
    image[e.env_off[9] + 97 + 5] ^= 0x04              # a forged ciphertext byte
    out, status, olen = env_open(e, image, in_len=in_len)
    failed = {2, 5, 9}
    assert status == [ECIES if o in failed else 0 for o in range(e.count)]
    assert olen == [0 if o == 2 else n for o, n in enumerate(e.lens)]
    want = e.plain_image(0x5A, zero={5, 9})  # (the short one has no output range: its bytes keep the fill)
    want[e.in_off[2]:e.in_off[2] + e.lens[2]] = 0x5A
    assert np.array_equal(out, want)
    # a wrong secret key fails every envelope with bytes to authenticate, and alone those
    out, status, _ = env_open(e, e.env_image(0x3C), secret=bytes(range(2, 34)))
    assert status == [ECIES] * e.count
    assert np.array_equal(out, e.plain_image(0x5A, zero=set(range(e.count))))


def test_seals_without_injection_differ_and_both_open(gpu, envelopes):
    e = envelopes
    a, _ = env_seal(e, inject=False)
    b, _ = env_seal(e, inject=False)
    for o in range(e.count):
        ea, eb = (bytes(x[e.env_off[o]:e.env_off[o] + e.lens[o] + 97]) for x in (a, b))
        assert ea[:65] != eb[:65] and ea[65:81] != eb[65:81] and ea[0] == 4
    for image in (a, b):
        out, status, _ = env_open(e, image)
        assert status == [0] * e.count and np.array_equal(out, e.plain_image(0x5A))


# ---- formats 13, 9 and 5 in one call: against orc_encode_full (all in C, with
# the injected values) and against chip_encode with the same injection

OBJ_SIZES = [0, 1, 15, 16, 17, 100, 926, 927, 928, 1023, 1024, 1025, 3999, 4000, 4096 - 97, 4096, 5000, 8191, 8192,
             8192 - 97, 12345, 16384 - 97, 16384, 20000, 32768 - 97, 32768, 40000, 65536 - 97, 65536, 65537, 70001,
             100000, 131072 - 97, 131072, 200000, 262144 - 97, 300001, 524288 - 97, 524288, (1 << 20) - 97, 1 << 20]


class Objects(Envelopes):
    def __init__(self, fmt, sizes, seed):
        from carbonado_amd import device as D
        super().__init__(sizes, seed)
        self.fmt = fmt
        self.out_off, self.need, self.total = D.ragged_layout(fmt & 12, [n + 97 for n in sizes], 256)

    def encode(self, inject=True):
        from carbonado_amd import device as D
        out = torch.full((self.total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        hashes = torch.full((self.count, 32), 0xEE, dtype=torch.uint8, device="cuda")
        scratch = D.ecies_ragged_scratch(self.fmt, self.lens)
        olen, info = D.encode_ragged_ecies(self.fmt, self.pub, dev(self.plain_image(0x11)), self.in_off, self.lens, out,
                                           self.out_off, hashes, scratch, inject=self.inject if inject else None)
        torch.cuda.synchronize()
        return out, hashes, olen, info

    def decode(self, out, hashes, olen, pads, secret=SECRET):
        from carbonado_amd import device as D
        back = torch.full((self.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.full((self.count,), 0x7777, dtype=torch.int32, device="cuda")
        scratch = D.ecies_ragged_scratch(self.fmt, olen, decode=True)
        plen = D.decode_ragged_ecies(self.fmt, secret, out, self.out_off, olen, hashes, pads, back, self.in_off, status,
                                     scratch)
        torch.cuda.synchronize()
        return back.cpu().numpy(), status.cpu().numpy().tolist(), plen


def _same_info(got, want: dict):
    for f, w in want.items():
        g = getattr(got, f)
        if isinstance(w, float) and math.isfinite(w):
            assert abs(g - w) <= 1e-6 * max(1.0, abs(w)), (f, g, w)
        else:  # integers; nan and inf for an empty input (0 / 0, x / 0), as the reference's f32 division gives
            assert g == w or (math.isnan(g) and math.isnan(w)), (f, g, w)


@pytest.mark.parametrize("fmt", [13, 9, 5])
def test_one_call_encode_equals_the_oracle_and_chip_encode_and_round_trips(gpu, fmt):
    import carbonado_amd as ca
    from oracle import oracle as O
    s = Objects(fmt, OBJ_SIZES, seed=31 + fmt)
    out, hashes, olen, info = s.encode()
    host, hh = out.cpu().numpy(), hashes.cpu().numpy()
    for o in range(s.count):
        sk, nonce = s.inject[o]
        enc, h, winfo = O.c_encode_full(s.pt[o], fmt, s.pub, sk, nonce)
        assert olen[o] == len(enc) == s.need[o], o
        assert bytes(host[s.out_off[o]:s.out_off[o] + olen[o]]) == enc, (o, s.lens[o])
        assert bytes(hh[o]) == h, o
        _same_info(info[o], winfo)
        if o % 5 == 0:
            cenc, ch, cinfo = ca.encode(s.pub, s.pt[o], fmt, ephemeral_sk=sk, nonce=nonce)
            assert cenc == enc and ch == h
            _same_info(info[o], {f: getattr(cinfo, f) for f in winfo})
    back, status, plen = s.decode(out, hashes, olen, [i.padding_len for i in info])
    assert status == [0] * s.count and plen == s.lens
    assert np.array_equal(back, s.plain_image(0x5A))
    # without injection two encodings of one input differ, and both decode
    out2, hashes2, olen2, info2 = s.encode(inject=False)
    assert olen2 == olen and not torch.equal(out2, out)
    back, status, _ = s.decode(out2, hashes2, olen2, [i.padding_len for i in info2])
    assert status == [0] * s.count and np.array_equal(back, s.plain_image(0x5A))


def test_damage_gives_the_bao_status_and_a_forged_envelope_the_ecies_one(gpu):
    from carbonado_amd import device as D
    s = Objects(13, [5000, 0, 70001, 1024, 20000, 300], seed=41)
    out, hashes, olen, info = s.encode()
    pads = [i.padding_len for i in info]
    out[s.out_off[2] + olen[2] // 2] ^= 0x20           # a damaged stream byte: bao's status, not ecies'
    # object 4: a stream re-encoded at level 12 over a forged envelope (every hash in it is right)
    env = np.frombuffer(s.env[4], dtype=np.uint8).copy()
    env[97 + 1234] ^= 0x01
    e_dev, scratch12 = dev(env), D.ragged_scratch(12, [env.size])
    h4 = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
    l4, _ = D.encode_ragged(12, e_dev, [0], [env.size], out, [s.out_off[4]], h4, scratch12)
    assert l4 == [olen[4]]
    hashes[4] = h4[0]
    back, status, plen = s.decode(out, hashes, olen, pads)
    assert status == [0, 0, 5, 0, ECIES, 0] and plen == s.lens
    assert np.array_equal(back, s.plain_image(0x5A, zero={2, 4}))
    # a wrong secret key: every object fails as ecies, none as bao
    back, status, _ = s.decode(out, hashes, olen, pads, secret=bytes(range(3, 35)))
    assert status == [ECIES, ECIES, 5, ECIES, ECIES, ECIES]
    assert np.array_equal(back, s.plain_image(0x5A, zero=set(range(6))))


def test_one_object_of_16_mib_less_97_at_13(gpu):
    from oracle import oracle as O
    s = Objects(13, [(16 << 20) - 97], seed=43)
    out, hashes, olen, info = s.encode()
    sk, nonce = s.inject[0]
    enc, h, winfo = O.c_encode_full(s.pt[0], 13, s.pub, sk, nonce)
    assert olen == [len(enc)] and bytes(hashes.cpu().numpy()[0]) == h
    assert bytes(out.cpu().numpy()[s.out_off[0]:s.out_off[0] + olen[0]]) == enc
    _same_info(info[0], winfo)
    back, status, plen = s.decode(out, hashes, olen, [info[0].padding_len])
    assert status == [0] and plen == s.lens and np.array_equal(back, s.plain_image(0x5A))


def test_level_13_streams_are_level_12_streams_to_the_read_and_audit_calls(gpu):
    """read_ranges and verify_slices take the streams of encode_ragged_ecies at
    13 as the level-12 streams (of the envelopes) they are."""
    from carbonado_amd import device as D
    s = Objects(13, [5000, 70001, 20000], seed=47)
    out, hashes, olen, info = s.encode()
    pads, cls = [i.padding_len for i in info], [i.chunk_len for i in info]
    rs, start, length = [0, 1, 2, 1], [0, 97, 19000, 65000], [300, 4096, 1097, 5098]  # two end with their envelope
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
        assert bytes(host[coff[r]:coff[r] + length[r]]) == s.env[rs[r]][start[r]:start[r] + length[r]], r
    # the first slice of every stream: the first 1024 bytes of shard 0, that is of the envelope
    rs, idx, cnt = [0, 1, 2], [0, 0, 0], [1, 1, 1]
    _, _, coff, clen, _, ct = D.slice_layout([8 * c for c in cls], idx, cnt)
    content = torch.full((ct + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((3,), 0x7777, dtype=torch.int32, device="cuda")
    got = D.verify_slices(out, s.out_off, olen, hashes, rs, idx, cnt, content, coff, status, D.audit_scratch(3, 3))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 3 and got == [1024] * 3
    host = content.cpu().numpy()
    for r in range(3):
        assert min(cls) >= 1024 and bytes(host[coff[r]:coff[r] + 1024]) == s.env[r][:1024], r
