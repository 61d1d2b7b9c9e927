"""CPU tests of the agree boundary (include/carbonado_hip_agree.h): the text
the KY kernels compile (carbonado_amd/csrc/agree_device.hpp) as a stand-alone
program under ASan + UBSan against Python integers, the Python oracle's
secp256k1 and hashlib, walked lane by lane as the kernels split the work; the
hybrid-key rule against the library's own host decode; and the boundary: the
chipy_* symbols beside the fourteen older sets, their ctypes and Rust bindings,
the errors the calls decide before they touch a device, in the header's order,
the scratch lengths and the bench tool's dry run."""
import ctypes
import hashlib
import hmac
import json
import random
import re
import subprocess
import sys
from pathlib import Path

import pytest

import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib
from oracle import host_oracle as H

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "carbonado_hip_agree.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_agree.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"
CSRC = ROOT / "carbonado_amd" / "csrc"
P, N = H.P, H.N
G = (H.GX, H.GY)

OK, INVALID_ARG, HASH_DECODE, ECIES, NO_DEVICE = 0, 1, 4, 17, 100

# small and sparse scalars leave most comb picks and ladder accumulators at infinity
SCALARS = [1, 2, 3, 15, 16, 17, N - 1, N - 2, (N - 1) // 2, 1 << 128, (1 << 128) - 1, 1 << 252, 1 << 255,
           int("0f" * 32, 16), int("f0" * 32, 16)]


def scalars():
    rng = random.Random(5)
    return SCALARS + [rng.randrange(1, N) for _ in range(12)]


def bases():
    return [G, H.point_mul(0xC0FFEE), H.point_mul(N - 1), H.point_mul(2)]


def hkdf(ikm: bytes) -> bytes:
    """HKDF-SHA256 without salt or info, 32 bytes, from hashlib and hmac alone."""
    prk = hmac.new(b"\0" * 32, ikm, hashlib.sha256).digest()
    return hmac.new(prk, b"\x01", hashlib.sha256).digest()


def field_edges():
    fold = 0x1000003D1
    vals = [0, 1, P - 1, P, P + 1, (1 << 256) - 1, fold, P - fold, (1 << 256) - fold]
    vals += [0xFFFFFFFF << (32 * i) for i in range(8)]  # all-ones limbs in every position of the 32-bit radix
    rng = random.Random(7)
    return vals + [rng.getrandbits(256) for _ in range(40)]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "agree_device_check.cpp", include=[CSRC])


def answers(exe, tmp_path, lines):
    f = tmp_path / "vectors.txt"
    f.write_text("\n".join(lines) + "\n")
    out = B.run_check(exe, str(f), timeout=600).splitlines()
    assert out[-1] == "0 failures"
    rows = [ln.split() for ln in out[:-1] if not ln.startswith("#")]
    assert len(rows) == len(lines)
    return rows


def test_field_ops_match_python(check, tmp_path):
    """Every operation takes any value below 2^256 as it is (weakly reduced): that
    is the largest magnitude the point formulas can feed in."""
    vals = field_edges()
    rng = random.Random(11)
    pairs = [(a, b) for a in vals[:17] for b in vals[:17]] + [(rng.choice(vals), rng.choice(vals)) for _ in range(300)]
    ops = {"mul": lambda a, b: a * b, "sqr": lambda a, b: a * a, "add": lambda a, b: a + b, "sub": lambda a, b: a - b,
           "mul21": lambda a, b: 21 * a, "mul8": lambda a, b: 8 * a, "norm": lambda a, b: a,
           "iszero": lambda a, b: int(a % P == 0), "cmov": lambda a, b: b}
    lines, want = [], []
    for a, b in pairs:
        for op, f in ops.items():
            lines.append("fe %s %064x %064x" % (op, a, b))
            want.append(f(a, b) % P)
    for a in vals:
        lines.append("fe inv %064x %064x" % (a, 0))
        want.append(pow(a, P - 2, P))
    got = answers(check, tmp_path, lines)
    for line, w, g in zip(lines, want, got):
        assert int(g[0], 16) == w, line


@pytest.fixture(scope="module")
def shared_points():
    """k B for every scalar and base, from the oracle, once."""
    return {(k, b): H.point_mul(k, b) for k in scalars() for b in bases()}


def test_seal_wave_matches_oracle(check, tmp_path, shared_points):
    """k G and k P as a wave computes them (64 comb picks, the butterfly, one
    inversion) and the key HKDF makes of them."""
    cases = [(k, b) for b in bases() for k in scalars()]
    got = answers(check, tmp_path, ["seal %064x %064x %064x" % (k, b[0], b[1]) for k, b in cases])
    for (k, b), g in zip(cases, got):
        eph, shared = H.ser_uncompressed(shared_points[(k, G)]), H.ser_uncompressed(shared_points[(k, b)])
        assert g[0] == eph.hex() and g[1] == shared[1:].hex(), (hex(k), b)
        assert g[2] == hkdf(eph + shared).hex() == H.hkdf_sha256(eph + shared).hex(), (hex(k), b)


def test_open_lane_matches_oracle(check, tmp_path, shared_points):
    """sk R as a lane computes it (16 multiples in the interleaved scratch, 64
    fixed windows) for R in 0x04 form and in both hybrid forms."""
    cases = [(k, b, 4) for b in bases() for k in scalars()]
    cases += [(k, b, 6 + (b[1] & 1)) for b in bases() for k in scalars()[:3]]
    ser = lambda b, tag: bytes([tag]) + H.ser_uncompressed(b)[1:]  # noqa: E731
    got = answers(check, tmp_path, ["open %064x %s" % (k, ser(b, tag).hex()) for k, b, tag in cases])
    for (k, b, tag), g in zip(cases, got):
        want = hkdf(ser(b, tag) + H.ser_uncompressed(shared_points[(k, b)]))
        assert g == ["0", want.hex()], (hex(k), b, tag)


def _oracle_parses(b: bytes) -> bool:
    try:
        H.parse_pubkey(b)
        return True
    except ValueError:
        return False


def test_key_parsing(check, tmp_path):
    q = H.point_mul(0xC0FFEE)
    x, y = q
    be = lambda v: v.to_bytes(32, "big")  # noqa: E731
    good = b"\x04" + be(x) + be(y)
    xs = next(v for v in range(1, 100) if pow((v ** 3 + 7) % P, (P - 1) // 2, P) == 1)  # x with x + p below 2^256 on the curve
    ys = pow((xs ** 3 + 7) % P, (P + 1) // 4, P)
    bad = {"x = p": b"\x04" + be(P) + be(y), "y off the curve": b"\x04" + be(x) + be(y ^ 1),
           "y = p - y swapped x": b"\x04" + be(y) + be(x), "x + p": b"\x04" + be(xs + P) + be(ys),
           "y + p": b"\x04" + be(xs) + be(ys + P) if ys + P < 1 << 256 else b"\x04" + be(x) + be(P),
           "prefix 00": b"\x00" + good[1:], "prefix 02": b"\x02" + good[1:], "prefix 03": b"\x03" + good[1:],
           "prefix 05": b"\x05" + good[1:], "hybrid wrong parity": bytes([7 - (y & 1)]) + good[1:],
           "zeros": bytes(65), "x = 0, y = 0 tagged": b"\x04" + bytes(64)}
    fine = {"full": good, "hybrid": bytes([6 + (y & 1)]) + good[1:], "small x": b"\x04" + be(xs) + be(ys),
            "negated": b"\x04" + be(x) + be(P - y)}
    names = list(bad) + list(fine)
    got = answers(check, tmp_path, ["open %064x %s" % (3, {**bad, **fine}[n].hex()) for n in names])
    for n, g in zip(names, got):
        if n in bad:
            assert g == ["17", "00" * 32], n
        else:
            assert g[0] == "0" and g[1] != "00" * 32, n
        # the oracle's parser (the reference's rule for 0x04) agrees wherever it has a say
        if {**bad, **fine}[n][0] == 4:
            assert _oracle_parses({**bad, **fine}[n]) == (n in fine), n


def test_hybrid_rule_is_the_host_decoders():
    """What the device accepts as a hybrid key (0x06 / 0x07: on the curve, the
    prefix's low bit equal to y's) is what the library's host decode, which takes
    those forms through OpenSSL, accepts: a hand-made hybrid envelope opens with
    the right parity and is refused with the wrong one."""
    import carbonado_amd as ca
    sk = (0x1234567).to_bytes(32, "big")
    pk = H.public_key(sk)
    eph_sk = (0xABCDEF01).to_bytes(32, "big")
    e = H.point_mul(int.from_bytes(eph_sk, "big"))
    shared = H.point_mul(int.from_bytes(eph_sk, "big"), H.parse_pubkey(pk))
    msg, nonce = b"hybrid envelopes are rare", bytes(range(16))
    for tag in (6, 7):
        eph = bytes([tag]) + H.ser_uncompressed(e)[1:]
        key = hkdf(eph + H.ser_uncompressed(shared))
        ct, t = H.aes256_gcm_encrypt(key, nonce, msg)
        env = eph + nonce + t + ct
        if tag == 6 + (e[1] & 1):
            assert ca.decoding.ecies(env, sk) == msg
        else:
            with pytest.raises(Exception):
                ca.decoding.ecies(env, sk)


def test_hkdf_rfc5869_and_hashlib(check, tmp_path):
    rng = random.Random(13)
    msgs = [bytes([0x0b] * 22), b"", b"a", bytes(55), bytes(56), bytes(63), bytes(64), bytes(119), bytes(120)]
    for _ in range(6):
        m = bytearray(rng.randbytes(130))
        m[65] = 4
        msgs.append(bytes(m))
    got = answers(check, tmp_path, ["hkdf %s" % (m.hex() or "-") for m in msgs])
    # RFC 5869 test case 3 (no salt, no info): the first 32 of its 42 bytes of OKM
    assert got[0][0] == "8da4e775a563c18f715f802a063c5a31b8a11f5c5ee1879ec3454e5f3c738d2d"
    for m, g in zip(msgs, got):
        assert g[0] == hkdf(m).hex(), len(m)
        if len(m) == 130:
            assert g[1] == g[0]  # hkdf_points: the same bytes assembled from limbs


def test_scalar_rule(check, tmp_path):
    ks = [0, 1, N - 1, N, N + 1, (1 << 256) - 1, 1 << 255, N - (1 << 128), N + (1 << 128)]
    got = answers(check, tmp_path, ["scalar %064x" % k for k in ks])
    assert [int(g[0]) for g in got] == [int(0 < k < N) for k in ks]


# ---- the boundary ---------------------------------------------------------------------------------------------

NAMES = {"chipy_abi_version", "chipy_keys_scratch_len", "chipy_seal_keys_dev", "chipy_open_keys_dev",
         "chipy_envelope_scratch_len", "chipy_seal_ragged_dev", "chipy_open_ragged_dev", "chipy_encode_scratch_len",
         "chipy_decode_scratch_len", "chipy_encode_ragged_dev", "chipy_decode_ragged_dev",
         "chipy_key_table_scratch_len", "chipy_key_table_dev"}
# the fifteenth boundary; boundary.BOUNDARIES holds the first nine
MINE = B._boundary("chipy_", "agree", _lib.AGREE_SIGNATURES, 13)
OLDER = B.BOUNDARIES + (B._boundary("chipf_", "fread", _lib.FREAD_SIGNATURES, 7),
                        B._boundary("chipq_", "qread", _lib.QREAD_SIGNATURES, 6),
                        B._boundary("chipk_", "kread", _lib.KREAD_SIGNATURES, 6),
                        B._boundary("chipg_", "gread", _lib.GREAD_SIGNATURES, 5),
                        B._boundary("chipp_", "paudit", _lib.PAUDIT_SIGNATURES, 8))


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipy_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == MINE.exports
    exported = B.exported()
    assert set(protos) == B.exports_of(exported, MINE.prefix) == set(MINE.signatures)
    for name, (_, ps) in protos.items():
        assert len(MINE.signatures[name][1]) == len(ps), name
    assert _lib.lib().chipy_abi_version() == 1
    assert "#define CHIPY_ABI_VERSION 1" in HEADER.read_text()
    # every older boundary keeps its count; no prefix clashes, no shared name
    assert [b.exports for b in OLDER] == [62, 5, 6, 4, 4, 3, 10, 10, 8, 7, 6, 6, 5, 8]
    for b in OLDER:
        assert len(B.exports_of(exported, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(MINE.prefix) and not MINE.prefix.startswith(b.prefix)
        assert not set(MINE.signatures) & set(b.signatures), b.prefix
    # the envelope and one-call forms have the argument lists of their chipe_ counterparts
    ecies = B.prototypes(ROOT / "include" / "carbonado_hip_ecies.h", "chipe_")
    for name in ("seal_ragged_dev", "open_ragged_dev", "encode_scratch_len", "decode_scratch_len", "encode_ragged_dev",
                 "decode_ragged_dev"):
        assert protos["chipy_" + name] == ecies["chipe_" + name], name
    names = lambda f: [n for n, _ in protos[f][1]]  # noqa: E731
    tail = ["d_scratch", "scratch_len", "stream"]
    assert names("chipy_seal_keys_dev") == ["pubkey", "pubkey_len", "eph_sk", "count", "d_pub", "pub_pitch", "d_keys",
                                            "key_pitch"] + tail
    assert names("chipy_open_keys_dev") == ["secret_key", "sk_len", "d_eph", "eph_pitch", "count", "d_keys", "key_pitch",
                                            "d_status"] + tail
    assert names("chipy_key_table_dev") == ["d_table", "info", "secret_key", "sk_len", "d_keytab", "keytab_len"] + tail


def test_ffi_agree_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipy_"), prototypes())
    assert re.search(r"pub const CHIPY_ABI_VERSION: c_int = 1;", B.ffi_text(FFI))


WRAPPERS = (("agree_scratch_len", "agree_scratch", ("chipy_keys_scratch_len",)),
            ("envelope_scratch_len", "envelope_scratch", ("chipy_envelope_scratch_len",)),
            ("seal_keys", "seal_keys", ("chipy_seal_keys_dev",)),
            ("open_keys", "open_keys", ("chipy_open_keys_dev",)),
            ("ecies_seal_ragged_dev_keys", "ecies_seal_ragged_dev_keys", ("chipy_seal_ragged_dev",)),
            ("ecies_open_ragged_dev_keys", "ecies_open_ragged_dev_keys", ("chipy_open_ragged_dev",)),
            ("ecies_ragged_scratch_len_dev_keys", "ecies_ragged_scratch_dev_keys",
             ("chipy_encode_scratch_len", "chipy_decode_scratch_len")),
            ("encode_ragged_ecies_dev_keys", "encode_ragged_ecies_dev_keys", ("chipy_encode_ragged_dev",)),
            ("decode_ragged_ecies_dev_keys", "decode_ragged_ecies_dev_keys", ("chipy_decode_ragged_dev",)),
            ("key_table_from_streams_scratch_len", "key_table_from_streams", ("chipy_key_table_scratch_len",)),
            ("key_table_from_streams", "key_table_from_streams", ("chipy_key_table_dev",)))


def test_lib_rs_and_device_module_have_the_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^mod ffi_agree;", lib, flags=re.M) and "chipy_abi_version" in lib
    for rust_fn, py_fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {rust_fn}\(", lib)
        assert m, rust_fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert re.search(rf"^def {py_fn}\(", src, flags=re.M), py_fn
        for call in calls:
            assert f"ffi_agree::{call}(" in body, (rust_fn, call)
            assert f"{call}" in src, call


# never dereferenced: the checks come first
IN, OUT, PUB, KEYS, STAT, SCR, HASH = 0x10000000, 0x40000000, 0x50000000, 0x60000000, 0x74000000, 0x78000000, 0x70000000
SK = bytes(range(1, 33))
N_BE = N.to_bytes(32, "big")


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def _u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs)


def test_scratch_lengths():
    L = _lib.lib()
    assert L.chipy_keys_scratch_len(0) == 0 == L.chipy_keys_scratch_len(1 << 31)
    for count in (1, 63, 64, 65, 130, 16384):
        s = L.chipy_keys_scratch_len(count)
        # the receiver's comb table, 16 x 96 B per object rounded up to a wave, the scalars
        assert s == 64 * 16 * 96 + -(-count // 64) * 64 * 1536 + 32 * count and s % 16 == 0
    lens = [100, 0, 8193, 16]
    g = L.chipe_gcm_scratch_len(_u64(lens), 4)
    assert L.chipy_envelope_scratch_len(_u64(lens), 4) == g + L.chipy_keys_scratch_len(4)
    assert L.chipy_envelope_scratch_len(_u64([]), 0) == 0 == L.chipy_envelope_scratch_len(None, 3)
    assert L.chipy_envelope_scratch_len(_u64([(1 << 36) - 31]), 1) == 0
    for fmt in (5, 9, 13):
        e, d = L.chipy_encode_scratch_len(fmt, _u64(lens), 4), L.chipy_decode_scratch_len(fmt, _u64([2000, 4000]), 2)
        assert e == L.chipe_encode_scratch_len(fmt, _u64(lens), 4) + L.chipy_keys_scratch_len(4) and e % 16 == 0
        assert d == L.chipe_decode_scratch_len(fmt, _u64([2000, 4000]), 2) + L.chipy_keys_scratch_len(2)
    for fmt in (0, 1, 4, 12, 7, 15, 16):
        assert L.chipy_encode_scratch_len(fmt, _u64(lens), 4) == 0 == L.chipy_decode_scratch_len(fmt, _u64(lens), 4)


def test_raw_key_calls_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    pk = H.public_key(SK)
    need = L.chipy_keys_scratch_len(5)

    def seal(pubkey=pk, eph=None, count=5, pub=PUB, pp=65, keys=KEYS, kp=32, scr=SCR, slen=need):
        return L.chipy_seal_keys_dev(pubkey, len(pubkey) if pubkey else 0, eph, count, pub, pp, keys, kp, scr, slen, None)

    def open_(sk=SK, eph=PUB, ep=65, count=5, keys=KEYS, kp=32, stat=STAT, scr=SCR, slen=need):
        return L.chipy_open_keys_dev(sk, len(sk) if sk else 0, eph, ep, count, keys, kp, stat, scr, slen, None)

    assert seal(count=0, pubkey=None, pub=None, keys=None, scr=None, slen=0, pp=0, kp=0) == OK
    assert open_(count=0, sk=None, eph=None, keys=None, stat=None, scr=None, slen=0, ep=0, kp=0) == OK
    for kw in (dict(pubkey=None), dict(pub=None), dict(keys=None), dict(scr=None), dict(count=1 << 31, slen=1 << 62),
               dict(pp=64), dict(kp=31), dict(pp=(1 << 32) + 1), dict(kp=(1 << 32) + 1), dict(scr=SCR + 8),
               dict(slen=need - 1)):
        assert seal(**kw) == INVALID_ARG, kw
    for kw in (dict(sk=None), dict(eph=None), dict(keys=None), dict(stat=None), dict(scr=None),
               dict(count=1 << 31, slen=1 << 62), dict(ep=64), dict(kp=31), dict(scr=SCR + 8), dict(slen=need - 1)):
        assert open_(**kw) == INVALID_ARG, kw
    good = b"".join((k + 1).to_bytes(32, "big") for k in range(5))
    for bad in (bytes(32), N_BE, b"\xff" * 32):  # 0, n, above n
        assert seal(eph=good[:64] + bad + good[96:]) == ECIES
        assert open_(sk=bad) == ECIES
    assert open_(sk=SK[:31]) == ECIES and open_(sk=SK + b"\0") == ECIES
    assert seal(pubkey=b"\x04" + bytes(64)) == ECIES and seal(pubkey=pk[:40]) == ECIES
    # the order: INVALID_ARG before the keys, the receiver key before the injected secrets, all before the device
    assert seal(pubkey=b"\x04" + bytes(64), slen=need - 1) == INVALID_ARG and open_(sk=N_BE, kp=31) == INVALID_ARG
    if last:
        assert seal() == last and seal(eph=good) == last and open_() == last
        assert seal(pubkey=H.ser_compressed(H.parse_pubkey(pk))) == last and open_(sk=(N - 1).to_bytes(32, "big")) == last
        assert seal(pp=96, kp=48, slen=need + 100) == last


def test_envelope_and_one_call_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    pk = H.public_key(SK)
    lens, in_off, env_off = [100, 0, 8193, 16], [0, 112, 112, 8320], [0, 208, 320, 8624]
    count = 4
    keep = []

    def inject(sks):
        arr = (_lib.EciesInjectC * count)()
        for o, sk in enumerate(sks):
            bs, bn = ctypes.create_string_buffer(sk, 32), ctypes.create_string_buffer(bytes(16), 16)
            keep.extend([bs, bn])
            arr[o].ephemeral_sk, arr[o].nonce = ctypes.addressof(bs), ctypes.addressof(bn)
        return arr

    def seal(pubkey=pk, inj=None, d_in=IN, n=lens, out=OUT, out_off=env_off, scr=SCR, cnt=count):
        return L.chipy_seal_ragged_dev(pubkey, len(pubkey) if pubkey else 0, inj, d_in, _u64(in_off), _u64(n), cnt, out,
                                       _u64(out_off), scr, None)

    def open_(sk=SK, d_in=OUT, in_len=None, out=IN, stat=STAT, scr=SCR, cnt=count):
        got = _u64([9] * count)
        rc = L.chipy_open_ragged_dev(sk, len(sk) if sk else 0, d_in, _u64(env_off), _u64(in_len or [n + 97 for n in lens]),
                                     cnt, out, _u64(in_off), got, stat, scr, None)
        return rc, list(got)

    assert seal(cnt=0) == OK and open_(cnt=0)[0] == OK
    assert seal(pubkey=None) == INVALID_ARG and seal(out=None) == INVALID_ARG and seal(scr=None) == INVALID_ARG
    assert seal(scr=SCR + 8) == INVALID_ARG and seal(d_in=IN + 8) == INVALID_ARG
    assert seal(out_off=[0, 100, 320, 8624]) == INVALID_ARG  # two envelopes overlap
    assert seal(pubkey=pk[:40]) == ECIES
    scalars_ = [(k + 1).to_bytes(32, "big") for k in range(count)]
    for bad in (bytes(32), N_BE):
        assert seal(inj=inject(scalars_[:2] + [bad] + scalars_[3:])) == ECIES  # decided before the device is asked for
    assert seal(pubkey=pk[:40], scr=SCR + 8) == INVALID_ARG
    assert open_(sk=None)[0] == INVALID_ARG and open_(stat=None)[0] == INVALID_ARG and open_(scr=SCR + 8)[0] == INVALID_ARG
    assert open_(sk=N_BE)[0] == ECIES and open_(sk=SK[:31])[0] == ECIES
    if last:
        assert seal() == last and seal(inj=inject(scalars_)) == last
        rc, got = open_(in_len=[197, 96, 8290, 113])
        assert rc == last and got == [100, 0, 8193, 16]
    # the one-call forms refuse what the chipe_ forms refuse, with the same status
    for fmt in (0, 4, 12, 15):
        assert L.chipy_encode_ragged_dev(fmt, pk, 65, None, IN, _u64(in_off), _u64(lens), count, OUT, _u64(env_off),
                                         _u64([0] * 4), HASH, None, SCR, None) == INVALID_ARG
        assert L.chipy_decode_ragged_dev(fmt, SK, 32, OUT, _u64(env_off), _u64(lens), count, HASH, None, IN,
                                         _u64(in_off), _u64([0] * 4), STAT, SCR, None) == INVALID_ARG
    for fmt in (5, 9, 13):
        off, need, total = _u64([0] * 4), _u64([0] * 4), ctypes.c_uint64()
        assert L.chipx_ragged_layout(fmt & 12, _u64([n + 97 for n in lens]), count, 256, 0, off, need,
                                     ctypes.byref(total)) == OK
        args = (pk, 65, None, IN, _u64(in_off), _u64(lens), count, OUT, off, _u64([0] * 4))
        assert L.chipy_encode_ragged_dev(fmt, *args, HASH, None, SCR + 8, None) == INVALID_ARG
        assert L.chipy_encode_ragged_dev(fmt, *args, None, None, SCR, None) == INVALID_ARG
        assert L.chipy_encode_ragged_dev(fmt, pk[:40], 40, *args[2:], HASH, None, SCR, None) == \
            L.chipe_encode_ragged_dev(fmt, pk[:40], 40, *args[2:], HASH, None, SCR, None) == ECIES
        if last:
            assert L.chipy_encode_ragged_dev(fmt, *args, HASH, None, SCR, None) == last


def test_key_table_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    TAB, KT = 0x79000000, 0x7B000000
    info = _lib.TableInfo(66, 8, 1024, 0)
    need, klen = L.chipy_key_table_scratch_len(ctypes.byref(info)), L.chipk_key_table_len(66)
    assert need and need % 16 == 0 and L.chipy_key_table_scratch_len(None) == 0
    assert L.chipy_key_table_scratch_len(ctypes.byref(_lib.TableInfo(0, 8, 1024, 0))) == 0
    assert need >= 66 * 96 + L.chipq_read_scratch_len(ctypes.byref(info), 66, 81, 1) + L.chipy_keys_scratch_len(66)
    assert L.chipy_key_table_scratch_len(ctypes.byref(_lib.TableInfo(130, 8, 1024, 0))) > need

    def call(table=TAB, inf=info, sk=SK, kt=KT, ktlen=klen, scr=SCR, slen=need):
        return L.chipy_key_table_dev(table, ctypes.byref(inf) if inf else None, sk, len(sk) if sk else 0, kt, ktlen, scr,
                                     slen, None)

    assert call(inf=None) == INVALID_ARG
    assert call(inf=_lib.TableInfo(0, 0, 0, 0), table=None, sk=None, kt=None, scr=None, ktlen=0, slen=0) == OK
    for kw in (dict(table=None), dict(sk=None), dict(kt=None), dict(scr=None), dict(table=TAB + 8), dict(kt=KT + 8),
               dict(scr=SCR + 8), dict(ktlen=klen - 1), dict(slen=need - 1), dict(inf=_lib.TableInfo(1 << 31, 8, 1024, 0))):
        assert call(**kw) == INVALID_ARG, kw
    assert call(sk=N_BE) == ECIES and call(sk=bytes(32)) == ECIES and call(sk=SK[:31]) == ECIES
    assert call(sk=N_BE, slen=need - 1) == INVALID_ARG  # the order
    if last:
        assert call() == last and call(ktlen=klen + 16, slen=need + 5) == last


def test_agree_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "agree_bench.py"), "--dry"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "agree_bench" and res["dry_run"] is True and res["level"] == 13
    small, large = res["sets"]["1024x1MiB"], res["sets"]["16384x64KiB"]
    assert (small["objects"], small["object_bytes"]) == (1024, 1 << 20)
    assert (large["objects"], large["object_bytes"]) == (16384, 64 << 10) and small["plain_bytes"] == large["plain_bytes"]
    L = _lib.lib()
    for s in (small, large):
        assert s["keys_scratch_bytes"] == L.chipy_keys_scratch_len(s["objects"])
        assert s["envelope_scratch_bytes"] == s["gcm_scratch_bytes"] + s["keys_scratch_bytes"]
        assert s["copies_back"] == 0 and s["waits"] == 0
        assert s["launches"] == {"seal_keys": 1, "open_keys": 1, "seal": 5, "open": 6}
