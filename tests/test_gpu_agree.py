"""The Ecies key agreement on the device (include/carbonado_hip_agree.h): the
raw key calls against the Python oracle's secp256k1 and HKDF, the envelope
calls against chipe_seal_ragged_dev / chipe_open_ragged_dev and the oracle's
ecies_encrypt, the one-call forms at 13, 9 and 5 against the chipe_ forms with
the same injected values.  Every comparison is of whole buffers, so the bytes
between and behind the outputs (a canary fill) are checked with them, and after
every call the key regions of the scratch must read as zeros."""
import ctypes
import dataclasses
import random

import numpy as np
import pytest
import torch

from oracle import host_oracle as H
from read_world import dev, up16
from test_gpu_ecies_dev import SECRET, Envelopes, Objects, _same_info  # the batches of the Ecies GPU tests

pytestmark = pytest.mark.gpu

ECIES = 17
N, P = H.N, H.P
EDGE_SCALARS = [1, 2, 3, 15, 16, 17, N - 1, N - 2, (N - 1) // 2, 1 << 128, (1 << 128) - 1, 1 << 252, 1 << 255,
                int("0f" * 32, 16), int("f0" * 32, 16)]
COUNTS = [1, 63, 64, 65, 130]
be = lambda v: v.to_bytes(32, "big")  # noqa: E731


class Agreement:
    """130 ephemeral scalars (the edge set first), their public keys k G, the
    points k P shared with the receiver P = SECRET G, and the AES keys.  By
    symmetry SECRET (k G) = k P: one set of oracle multiplications serves the
    seal and the open."""

    def __init__(self):
        rng = random.Random(2027)
        self.ks = EDGE_SCALARS + [rng.randrange(1, N) for _ in range(130 - len(EDGE_SCALARS))]
        self.receiver = H.public_key(SECRET)
        peer = H.parse_pubkey(self.receiver)
        self.pub = [H.ser_uncompressed(H.point_mul(k)) for k in self.ks]
        self.shared = [H.ser_uncompressed(H.point_mul(k, peer)) for k in self.ks]
        self.keys = [H.hkdf_sha256(e + s) for e, s in zip(self.pub, self.shared)]
        self.sk_bytes = b"".join(be(k) for k in self.ks)


@pytest.fixture(scope="module")
def agreement():
    return Agreement()


def image(size, fill, pitch, rows):
    img = np.full(size, fill, dtype=np.uint8)
    for o, r in enumerate(rows):
        img[o * pitch:o * pitch + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return img


def keys_region_is_zero(scratch, count):
    """[sk, total) of an agreement scratch: 32 bytes per object at its end; the public tables in front stay"""
    s = scratch.cpu().numpy()
    return not s[s.size - 32 * count:].any() and s[:s.size - 32 * count].any()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("pitches", [(65, 32), (96, 48)])
def test_seal_keys_equal_the_oracle(gpu, agreement, count, pitches):
    from carbonado_amd import device as D
    a, (pp, kp) = agreement, pitches
    pub = torch.full((count * pp + 40,), 0xA5, dtype=torch.uint8, device="cuda")
    keys = torch.full((count * kp + 40,), 0x5A, dtype=torch.uint8, device="cuda")
    scratch = D.agree_scratch(count).fill_(0xEE)
    D.seal_keys(a.receiver, count, pub, pp, keys, kp, scratch, eph_sk=a.sk_bytes[:32 * count])
    torch.cuda.synchronize()
    assert np.array_equal(pub.cpu().numpy(), image(pub.numel(), 0xA5, pp, a.pub[:count]))
    assert np.array_equal(keys.cpu().numpy(), image(keys.numel(), 0x5A, kp, a.keys[:count]))
    assert keys_region_is_zero(scratch, count)


def test_seal_keys_from_the_rng_agree_with_open_keys(gpu, agreement):
    """Without injected secrets: valid points, different every time, and the
    receiver derives the same keys from them."""
    from carbonado_amd import device as D
    count = 70
    pubs, keyss = [], []
    for _ in range(2):
        pub = torch.zeros(count * 65, dtype=torch.uint8, device="cuda")
        keys = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
        scratch = D.agree_scratch(count).fill_(0xEE)
        D.seal_keys(agreement.receiver[1:], count, pub, 65, keys, 32, scratch)  # 64-byte form of the key
        torch.cuda.synchronize()
        assert keys_region_is_zero(scratch, count)
        pubs.append(pub)
        keyss.append(keys)
    back = torch.full((count * 32,), 0x77, dtype=torch.uint8, device="cuda")
    status = torch.full((count,), 0x7777, dtype=torch.int32, device="cuda")
    scratch = D.agree_scratch(count).fill_(0xEE)
    D.open_keys(SECRET, pubs[0], 65, count, back, 32, status, scratch)
    torch.cuda.synchronize()
    assert keys_region_is_zero(scratch, count)
    p0, p1 = (p.cpu().numpy().reshape(count, 65) for p in pubs)
    assert (p0[:, 0] == 4).all() and all(H.on_curve((int.from_bytes(bytes(r[1:33]), "big"),
                                                       int.from_bytes(bytes(r[33:]), "big"))) for r in p0[:5])
    assert not (p0 == p1).all(axis=1).any()
    assert status.cpu().tolist() == [0] * count and torch.equal(back, keyss[0]) and not torch.equal(back, keyss[1])


@pytest.mark.parametrize("count", COUNTS)
def test_open_keys_equal_the_oracle(gpu, agreement, count):
    from carbonado_amd import device as D
    a = agreement
    eph = dev(image(count * 81 + 7, 0x3C, 81, a.pub[:count]))
    keys = torch.full((count * 32 + 40,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((count + 2,), 0x7777, dtype=torch.int32, device="cuda")
    scratch = D.agree_scratch(count).fill_(0xEE)
    D.open_keys(SECRET, eph, 81, count, keys, 32, status, scratch)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * count + [0x7777] * 2
    assert np.array_equal(keys.cpu().numpy(), image(keys.numel(), 0x5A, 32, a.keys[:count]))
    assert keys_region_is_zero(scratch, 1) and not scratch.cpu().numpy()[-32 * count:].any()


def test_open_keys_under_the_edge_secrets(gpu):
    """One secret per batch: every edge scalar as the receiver's secret, over
    three ephemeral keys of which one is in the hybrid form."""
    from carbonado_amd import device as D
    pts = [H.point_mul(0xC0FFEE), H.point_mul(N - 1), H.point_mul(5)]
    eph = [H.ser_uncompressed(pts[0]), H.ser_uncompressed(pts[1]),
           bytes([6 + (pts[2][1] & 1)]) + H.ser_uncompressed(pts[2])[1:]]
    for k in EDGE_SCALARS:
        want = [H.hkdf_sha256(e + H.ser_uncompressed(H.point_mul(k, p))) for e, p in zip(eph, pts)]
        keys = torch.full((3 * 48,), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.full((3,), 0x7777, dtype=torch.int32, device="cuda")
        scratch = D.agree_scratch(3).fill_(0xEE)
        D.open_keys(be(k), dev(image(3 * 65, 0, 65, eph)), 65, 3, keys, 48, status, scratch)
        torch.cuda.synchronize()
        assert keys_region_is_zero(scratch, 3), hex(k)
        assert status.cpu().tolist() == [0, 0, 0], hex(k)
        assert np.array_equal(keys.cpu().numpy(), image(3 * 48, 0x5A, 48, want)), hex(k)


def test_keys_that_do_not_parse_fail_alone(gpu, agreement):
    from carbonado_amd import device as D
    a = agreement
    x, y = H.parse_pubkey(a.pub[20])
    good = a.pub[20]
    bad = {3: b"\x04" + be(P) + be(y), 17: b"\x04" + be(x) + be(y ^ 1), 63: b"\x00" + good[1:], 64: b"\x02" + good[1:],
           65: b"\x05" + good[1:], 66: bytes([7 - (y & 1)]) + good[1:], 129: b"\x04" + b"\xff" * 64}
    hybrid = bytes([6 + (y & 1)]) + good[1:]
    count = 130
    rows = [bad.get(o, hybrid if o == 100 else a.pub[o]) for o in range(count)]
    want = [bytes(32) if o in bad else a.keys[o] for o in range(count)]
    want[100] = H.hkdf_sha256(hybrid + a.shared[20])  # the HKDF input holds the prefix as the envelope does
    keys = torch.full((count * 32 + 40,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((count,), 0x7777, dtype=torch.int32, device="cuda")
    D.open_keys(SECRET, dev(image(count * 65, 0, 65, rows)), 65, count, keys, 32, status, D.agree_scratch(count))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [ECIES if o in bad else 0 for o in range(count)]
    assert np.array_equal(keys.cpu().numpy(), image(keys.numel(), 0x5A, 32, want))


# ---- envelopes: chipy_seal_ragged_dev / chipy_open_ragged_dev against the chipe_ calls and the oracle

ENV_LENS = [0, 1, 15, 16, 17, 8191, 8192, 8193, 2222, 777, 2999, 1500]


def gcm_key_region_is_zero(scratch, count, lens):
    """the GCM scratch's [keys, ok) and, behind the GCM scratch, the agreement's [sk, total)"""
    from carbonado_amd import _lib
    s = scratch.cpu().numpy()
    g = _lib.lib().chipe_gcm_scratch_len((ctypes.c_uint64 * count)(*lens), count)
    lo, hi = up16(48 * count) + 96 * count, g - up16(4 * count)
    return hi > lo and not s[lo:hi].any() and not s[s.size - 32 * count:].any() and s.size > g


@pytest.fixture(scope="module")
def envelopes():
    return Envelopes(ENV_LENS, seed=29, residues=(0, 3, 8, 15))


def y_seal(e, inject=True):
    from carbonado_amd import device as D
    out = torch.full((e.env_size,), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = D.envelope_scratch(e.lens).fill_(0xEE)
    D.ecies_seal_ragged_dev_keys(e.pub, dev(e.plain_image(0x11)), e.in_off, e.lens, out, e.env_off, scratch,
                                 inject=e.inject if inject else None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), scratch


def y_open(e, img, in_len=None, secret=SECRET):
    from carbonado_amd import device as D
    in_len = in_len or [n + 97 for n in e.lens]
    out = torch.full((e.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((e.count,), 0x7777, dtype=torch.int32, device="cuda")
    plain = [max(0, n - 97) for n in in_len]
    scratch = D.envelope_scratch(plain).fill_(0xEE)
    olen = D.ecies_open_ragged_dev_keys(secret, dev(img), e.env_off, in_len, out, e.in_off, status, scratch)
    torch.cuda.synchronize()
    assert gcm_key_region_is_zero(scratch, e.count, plain)
    return out.cpu().numpy(), status.cpu().numpy().tolist(), olen


def test_seal_equals_the_host_agreements_bytes_and_the_oracles(gpu, envelopes):
    from carbonado_amd import device as D
    e = envelopes
    out, scratch = y_seal(e)
    assert gcm_key_region_is_zero(scratch, e.count, e.lens)
    host = torch.full((e.env_size,), 0xA5, dtype=torch.uint8, device="cuda")
    D.ecies_seal_ragged(e.pub, dev(e.plain_image(0x11)), e.in_off, e.lens, host, e.env_off, D.gcm_scratch(e.lens),
                        inject=e.inject)
    torch.cuda.synchronize()
    assert np.array_equal(out, host.cpu().numpy())
    py = [H.ecies_encrypt(e.pub, p, sk, nonce) for p, (sk, nonce) in zip(e.pt, e.inject)]
    assert np.array_equal(out, e.env_image(0xA5, envs=py))


def test_open_returns_the_plaintext_and_failures_stay_alone(gpu, envelopes):
    e = envelopes
    out, status, olen = y_open(e, e.env_image(0x3C))
    assert status == [0] * e.count and olen == e.lens and np.array_equal(out, e.plain_image(0x5A))
    img = e.env_image(0x3C)
    in_len = [n + 97 for n in e.lens]
    img[e.env_off[3] + 81 + 7] ^= 0x10                # a tag byte
    img[e.env_off[6] + 40] ^= 0x01                    # the ephemeral key leaves the curve
    img[e.env_off[9]] = 0x02                          # a prefix no 65-byte key has
    in_len[10] = 96                                   # shorter than an envelope's overhead
    out, status, olen = y_open(e, img, in_len=in_len)
    failed = {3, 6, 9, 10}
    assert status == [ECIES if o in failed else 0 for o in range(e.count)]
    assert olen == [0 if o == 10 else n for o, n in enumerate(e.lens)]
    want = e.plain_image(0x5A, zero={3, 6, 9})
    want[e.in_off[10]:e.in_off[10] + e.lens[10]] = 0x5A  # (the short one has no output range: its bytes keep the fill)
    assert np.array_equal(out, want)
    out, status, _ = y_open(e, e.env_image(0x3C), secret=bytes(range(2, 34)))  # a wrong secret
    assert status == [ECIES] * e.count and np.array_equal(out, e.plain_image(0x5A, zero=set(range(e.count))))


def test_seals_without_injection_differ_and_the_host_path_opens_them(gpu, envelopes):
    from carbonado_amd import device as D
    e = envelopes
    a, _ = y_seal(e, inject=False)
    b, _ = y_seal(e, inject=False)
    for o in range(e.count):
        ea, eb = (bytes(x[e.env_off[o]:e.env_off[o] + e.lens[o] + 97]) for x in (a, b))
        assert ea[:65] != eb[:65] and ea[65:81] != eb[65:81] and ea[0] == 4
    out, status, _ = y_open(e, a)
    assert status == [0] * e.count and np.array_equal(out, e.plain_image(0x5A))
    back = torch.full((e.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((e.count,), 0x7777, dtype=torch.int32, device="cuda")
    D.ecies_open_ragged(SECRET, dev(b), e.env_off, [n + 97 for n in e.lens], back, e.in_off, st, D.gcm_scratch(e.lens))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * e.count and np.array_equal(back.cpu().numpy(), e.plain_image(0x5A))


# ---- formats 13, 9 and 5 in one call against the chipe_ forms

SIZES = [0, 1, 927, 4096 - 97, 5000, 1 << 20]


def one_call_key_regions_are_zero(scratch, env_rows, plain, count):
    """The scratch of a one-call form: envelope rows of up16(env_rows[o]) bytes, then the GCM scratch laid out
    for the plaintext lengths the call found, then the agreement's: [keys, ok) of the first and the 32 * count
    bytes of scalars at the end of the second must read as zeros, and both must lie inside the scratch."""
    from carbonado_amd import _lib
    L = _lib.lib()
    s = scratch.cpu().numpy()
    base = sum(up16(n) for n in env_rows)
    g = L.chipe_gcm_scratch_len((ctypes.c_uint64 * count)(*plain), count)
    a = L.chipy_keys_scratch_len(count)
    lo, hi = base + up16(48 * count) + 96 * count, base + g - up16(4 * count)
    end = base + g + a
    return (g > 0 and hi > lo and end <= s.size and not s[lo:hi].any() and not s[end - 32 * count:end].any()
            and s[base:lo].any())


class YObjects(Objects):
    def encode_y(self):
        from carbonado_amd import device as D
        out = torch.full((self.total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        hashes = torch.full((self.count, 32), 0xEE, dtype=torch.uint8, device="cuda")
        scratch = D.ecies_ragged_scratch_dev_keys(self.fmt, self.lens).fill_(0xEE)
        olen, info = D.encode_ragged_ecies_dev_keys(self.fmt, self.pub, dev(self.plain_image(0x11)), self.in_off,
                                                    self.lens, out, self.out_off, hashes, scratch, inject=self.inject)
        torch.cuda.synchronize()
        assert one_call_key_regions_are_zero(scratch, [n + 97 for n in self.lens], self.lens, self.count)
        return out, hashes, olen, info

    def decode_y(self, out, hashes, olen, pads, secret=SECRET):
        from carbonado_amd import device as D
        back = torch.full((self.in_size,), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.full((self.count,), 0x7777, dtype=torch.int32, device="cuda")
        scratch = D.ecies_ragged_scratch_dev_keys(self.fmt, olen, decode=True).fill_(0xEE)
        plen = D.decode_ragged_ecies_dev_keys(self.fmt, secret, out, self.out_off, olen, hashes, pads, back, self.in_off,
                                              status, scratch)
        torch.cuda.synchronize()
        # the rows are sized from the stream lengths, the GCM layout from the envelopes the call found in them
        assert one_call_key_regions_are_zero(scratch, olen, self.lens, self.count)
        return back.cpu().numpy(), status.cpu().numpy().tolist(), plen


@pytest.mark.parametrize("fmt", [13, 9, 5])
def test_one_call_forms_equal_the_host_agreements(gpu, fmt):
    s = YObjects(fmt, SIZES, seed=53 + fmt)
    out, hashes, olen, info = s.encode_y()
    hout, hhashes, holen, hinfo = s.encode()
    assert olen == holen and torch.equal(out, hout) and torch.equal(hashes, hhashes)
    for a, b in zip(info, hinfo):
        _same_info(a, dataclasses.asdict(b))
    pads = [i.padding_len for i in info]
    back, status, plen = s.decode_y(out, hashes, olen, pads)
    assert status == [0] * s.count and plen == s.lens and np.array_equal(back, s.plain_image(0x5A))
    # a damaged stream keeps the status the chipe_ decode gives it, the others open
    out[s.out_off[4] + olen[4] // 2] ^= 0x20
    back, status, plen = s.decode_y(out, hashes, olen, pads)
    hback, hstatus, hplen = s.decode(out, hashes, olen, pads)
    assert status == hstatus and plen == hplen and np.array_equal(back, hback)
    if fmt & 4:
        assert status[4] not in (0, ECIES) and status[:4] + status[5:] == [0] * 5
        assert np.array_equal(back, s.plain_image(0x5A, zero={4}))
    back, status, _ = s.decode_y(out, hashes, olen, pads, secret=bytes(range(3, 35)))
    assert status == s.decode(out, hashes, olen, pads, secret=bytes(range(3, 35)))[1]
    assert np.array_equal(back, s.plain_image(0x5A, zero=set(range(s.count))))


# ---- the resident key table without the host seeing a header or a key

def test_key_table_equals_the_host_made_one(gpu):
    """66 small streams: 64 at level 13, of which one has a flipped byte inside
    its first 81 envelope bytes (rebuilt and vouched: status 0), one has shards
    that contradict its tree (zfec of the envelope, a parity byte altered, bao
    over the eight shards as they are, then a flipped byte in chunk 0: the
    rebuilt chunk does not hash to its node, status 5) and one a damaged parent
    node above chunk 0 (the strict read's own refusal, as the host-made table
    records it), and two level-12 streams, one of an object shorter than 97
    bytes and one whose "envelope" does not start with a point (17 each)."""
    from bao_damage import chunk_off
    from carbonado_amd import device as D
    from oracle import oracle as O
    rng = np.random.default_rng(61)
    sizes = [int(x) for x in rng.integers(1, 3999, 64)]
    REBUILT, PARENT, CONTRA, SHORT, NOPOINT = 10, 11, 12, 64, 65
    sizes[REBUILT] = sizes[PARENT] = sizes[CONTRA] = 3999  # envelopes of 4096 bytes: 8 chunks, chunk i = shard i
    envs = [n + 97 for n in sizes] + [50, 300]
    count = len(envs)
    pitch = 4096
    plain = rng.integers(0, 256, 64 * pitch, dtype=np.uint8)
    inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
              for _ in sizes]
    off, _, total = D.ragged_layout(12, envs, 256)
    buf = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    hashes = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
    olen, infos = D.encode_ragged_ecies_dev_keys(13, O.c_public_key(SECRET), dev(plain), [o * pitch for o in range(64)],
                                                 sizes, buf, off[:64], hashes[:64],
                                                 D.ecies_ragged_scratch_dev_keys(13, sizes), inject=inject)
    raw = rng.integers(0, 256, 512, dtype=np.uint8)
    raw[64] = 0  # the second object's first byte: no 65-byte key starts with it
    olen12, infos12 = D.encode_ragged(12, dev(raw), [0, 64], envs[64:], buf, off[64:], hashes[64:],
                                      D.ragged_scratch(12, envs[64:]))
    torch.cuda.synchronize()
    lens, infos = olen + olen12, infos + infos12
    pads, cls = [i.padding_len for i in infos], [i.chunk_len for i in infos]
    assert cls[REBUILT] == cls[PARENT] == cls[CONTRA] == 1024 and pads[REBUILT] == pads[CONTRA] == 0
    # the contradiction: the same envelope sealed again, zfec, one byte of parity shard 4 altered, bao over the shards
    env = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    D.ecies_seal_ragged_dev_keys(O.c_public_key(SECRET), dev(plain), [CONTRA * pitch], [3999], env, [0],
                                 D.envelope_scratch([3999]), inject=[inject[CONTRA]])
    zoff, _, ztotal = D.ragged_layout(8, [4096], 256, 0)
    z = torch.zeros(ztotal, dtype=torch.uint8, device="cuda")
    zl, _ = D.encode_ragged(8, env, [0], [4096], z, zoff, torch.zeros((1, 32), dtype=torch.uint8, device="cuda"),
                            D.ragged_scratch(8, [4096]))
    assert zl == [8192]
    z[zoff[0] + 4 * 1024 + 10] ^= 0x01
    boff, _, btotal = D.ragged_layout(4, [8192], 256)
    b = torch.zeros(btotal, dtype=torch.uint8, device="cuda")
    bl, _ = D.encode_ragged(4, z, [zoff[0]], [8192], b, boff, hashes[CONTRA:CONTRA + 1], D.ragged_scratch(4, [8192]))
    assert bl == [lens[CONTRA]]
    buf[off[CONTRA]:off[CONTRA] + bl[0]] = b[boff[0]:boff[0] + bl[0]]
    # a header byte; chunk 0's CV in its parent; a byte of chunk 0 of the contradicted stream
    at = [off[REBUILT] + chunk_off(0, 8) + 40, off[PARENT] + chunk_off(0, 8) - 64 + 5, off[CONTRA] + chunk_off(0, 8) + 700]
    buf[torch.tensor(at, dtype=torch.int64, device="cuda")] ^= 0x10
    # the host-made table: one wait, the key agreements on the stage pool, two uploads
    keys, ivs, kstat = D.stream_keys(SECRET, buf, off, lens, hashes, pads, cls, D.stream_keys_scratch(count))
    want_status = [0] * count
    want_status[CONTRA], want_status[SHORT], want_status[NOPOINT] = 5, ECIES, ECIES
    want_status[PARENT] = int(kstat[PARENT])
    assert kstat.tolist() == want_status and want_status[PARENT] in (5, 7)  # the strict read's own refusal, not Ecies'
    host_made = D.key_table(keys, ivs, kstat)
    table = D.stream_table(buf, off, lens, hashes, pads, cls)
    need = D._lib.lib().chipy_key_table_scratch_len(ctypes.byref(table.info))
    scratch = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    kt = D.key_table_from_streams(table, SECRET, scratch[:need])
    torch.cuda.synchronize()
    assert kt.table.numel() == host_made.table.numel() and torch.equal(kt.table, host_made.table)
    s = scratch.cpu().numpy()
    assert not s[need - 32 * count:need].any() and (s[need:] == 0xEE).all()  # the secret is gone; nothing past the scratch
    # the planned plaintext read over either table: the same bytes and words
    rs = torch.arange(count, dtype=torch.int32, device="cuda")
    start = torch.zeros(count, dtype=torch.int64, device="cuda")
    length = torch.full((count,), 100, dtype=torch.int64, device="cuda")
    got = []
    for t in (kt, host_made):
        content = torch.full((count * 112,), 0xA5, dtype=torch.uint8, device="cuda")
        clen = torch.zeros(count, dtype=torch.int64, device="cuda")
        words = [torch.full((count,), 0x7777, dtype=torch.int32, device="cuda") for _ in range(3)]
        D.read_plain_ranges_planned(table, t, rs, start, length, 100, content, 112, clen, *words,
                                    D.planned_plain_read_scratch(table, count, 100), flags=1)
        torch.cuda.synchronize()
        got.append([x.cpu().numpy() for x in (content, clen, *words)])
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    status = got[0][2].tolist()
    assert status == want_status
    host = got[0][0]
    for o in (0, 5, REBUILT, 63):
        n = min(100, sizes[o])
        assert bytes(host[o * 112:o * 112 + n]) == bytes(plain[o * pitch:o * pitch + n]), o
    D.wipe_key_table(kt)
    torch.cuda.synchronize()
    assert not kt.table.any()
