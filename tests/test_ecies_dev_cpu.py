"""CPU tests of the ecies boundary (include/carbonado_hip_ecies.h): the chipe_*
symbols beside the six older sets, their ctypes and Rust bindings, every error
the calls decide before they touch a device, in the header's order, the scratch
length, the bench tool's dry run, and the arithmetic and host logic
(carbonado_amd/csrc/gcm_device.hpp, ecies_plan.hpp) as a stand-alone program
under ASan + UBSan, linked with libcrypto."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

import test_read_cpu as RC
import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "carbonado_hip_ecies.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_ecies.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

OK, INVALID_ARG, ECIES, NO_DEVICE = 0, 1, 17, 100
NAMES = {"chipe_abi_version", "chipe_gcm_scratch_len", "chipe_gcm_seal_ragged_dev", "chipe_gcm_open_ragged_dev",
         "chipe_seal_ragged_dev", "chipe_open_ragged_dev", "chipe_encode_scratch_len", "chipe_decode_scratch_len",
         "chipe_encode_ragged_dev", "chipe_decode_ragged_dev"}


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipe_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipe_")
    assert _lib.lib().chipe_abi_version() == 1
    assert "#define CHIPE_ABI_VERSION 1" in HEADER.read_text()
    # the six older boundaries keep their sets
    B.assert_older_keep_their_sets(exported, "chipe_")
    # the argument lists the issue fixes
    assert [n for n, _ in protos["chipe_seal_ragged_dev"][1]] == [
        "pubkey", "pubkey_len", "inject", "d_in", "in_off", "n", "count", "d_out", "out_off", "d_scratch", "stream"]
    assert [n for n, _ in protos["chipe_open_ragged_dev"][1]] == [
        "secret_key", "sk_len", "d_in", "in_off", "in_len", "count", "d_out", "out_off", "out_len", "d_status",
        "d_scratch", "stream"]


def test_older_entry_points_still_refuse_the_ecies_bit():
    """The seventh header adds; nothing about the Ecies bit changes elsewhere."""
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    got = (ctypes.c_uint64 * 1)()
    for fmt in (1, 5, 9, 13):
        assert L.chipx_encode_ragged_dev(fmt, 0x1000, u64([0]), u64([100]), 1, 0x2000, u64([0]), got, 0x3000, None,
                                         0x4000, None) == INVALID_ARG
        assert L.chipx_decode_ragged_dev(fmt, 0x1000, u64([0]), u64([1096]), 1, 0x3000, u32([0]), 0x2000, u64([0]), got,
                                         0x5000, 0x4000, None) == INVALID_ARG
        assert L.chip_encode_batch_dev(fmt, 0x1000, 1024, 1000, 1, 0x2000, 4096, got, 0x3000, None, 0x4000,
                                       None) == INVALID_ARG


def test_ffi_ecies_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipe_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPE_ABI_VERSION: c_int = 1;", text)


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_ecies;", lib, flags=re.M)
    for fn, call in (("gcm_scratch_len", "chipe_gcm_scratch_len"), ("gcm_seal_ragged", "chipe_gcm_seal_ragged_dev"),
                     ("gcm_open_ragged", "chipe_gcm_open_ragged_dev"), ("ecies_seal_ragged", "chipe_seal_ragged_dev"),
                     ("ecies_open_ragged", "chipe_open_ragged_dev"), ("encode_ragged_ecies", "chipe_encode_ragged_dev"),
                     ("decode_ragged_ecies", "chipe_decode_ragged_dev")):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert f"ffi_ecies::{call}(" in body, fn
    assert "chipe_abi_version" in lib


def test_device_module_has_the_bindings():
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    for fn in ("gcm_scratch", "gcm_seal_ragged", "gcm_open_ragged", "ecies_seal_ragged", "ecies_open_ragged",
               "encode_ragged_ecies", "decode_ragged_ecies"):
        assert re.search(rf"^def {fn}\(", src, flags=re.M), fn
    for call in NAMES - {"chipe_abi_version"}:
        assert f"{call}(" in src, call


# never dereferenced: the checks come first
IN, OUT, TAG, STAT, SCR = 0x10000000, 0x40000000, 0x70000000, 0x74000000, 0x78000000
LENS = [100, 0, 8193, 16]
IN_OFF = [0, 112, 112, 8320]
OUT_OFF = [1, 120, 130, 9000]
KEYS, IVS = bytes(range(128)), bytes(range(64))


def _need(lens=LENS):
    return _lib.lib().chipe_gcm_scratch_len(RC._u64(lens), len(lens))


def _raw(seal=True, keys=KEYS, ivs=IVS, d_in=IN, in_off=IN_OFF, lens=LENS, count=None, d_out=OUT, out_off=OUT_OFF,
         tag=TAG, stat=STAT, scratch=SCR, scratch_len=None, arrays=True):
    u64 = RC._u64
    L = _lib.lib()
    count = len(lens) if count is None else count
    scratch_len = _need(lens) if scratch_len is None else scratch_len
    k = ctypes.cast(ctypes.c_char_p(keys), _lib.c_u8p) if keys is not None else None
    v = ctypes.cast(ctypes.c_char_p(ivs), _lib.c_u8p) if ivs is not None else None
    n = u64(lens) if arrays else None
    if seal:
        return L.chipe_gcm_seal_ragged_dev(k, v, d_in, u64(in_off), n, count, d_out, u64(out_off), tag, scratch,
                                           scratch_len, None)
    # an open reads where the seal wrote: its plaintext side (16-B aligned) is the output
    return L.chipe_gcm_open_ragged_dev(k, v, d_out, u64(out_off), n, count, tag, d_in, u64(in_off), stat, scratch,
                                       scratch_len, None)


@pytest.mark.parametrize("seal", [True, False])
def test_raw_argument_errors_need_no_device(seal):
    import torch
    last = NO_DEVICE if not torch.cuda.is_available() else None

    def rc(**kw):
        return _raw(seal=seal, **kw)
    assert rc(count=0) == OK and rc(count=0, keys=None, ivs=None, arrays=False, scratch=None, tag=None) == OK
    assert rc(keys=None) == INVALID_ARG and rc(ivs=None) == INVALID_ARG and rc(arrays=False) == INVALID_ARG
    assert rc(tag=None) == INVALID_ARG and rc(scratch=None) == INVALID_ARG
    if not seal:
        assert rc(stat=None) == INVALID_ARG
    assert rc(count=1 << 31) == INVALID_ARG
    assert rc(lens=[100, 0, (1 << 36) - 31, 16], scratch_len=1 << 40) == INVALID_ARG
    assert rc(d_in=None) == INVALID_ARG and rc(d_out=None) == INVALID_ARG
    assert rc(in_off=[0, 112, (1 << 53) + 16, 8320]) == INVALID_ARG
    # the plaintext side wants 16-B alignment (an empty message has no address); the other side takes any
    assert rc(in_off=[8, 112, 112, 8320]) == INVALID_ARG and rc(d_in=IN + 4) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    # two output ranges that overlap: the ciphertexts of a seal, the plaintexts of an open
    if seal:
        assert rc(out_off=[1, 120, 100, 9000]) == INVALID_ARG
    else:
        assert rc(in_off=[0, 112, 96, 8320]) == INVALID_ARG
    assert rc(scratch_len=_need() - 1) == INVALID_ARG
    if last:
        assert rc() == last
        assert rc(in_off=[0, 8, 112, 8320]) == last      # (the empty message's offset is not looked at)
        assert rc(lens=[0, 0, 0, 0], d_in=None, d_out=None) == last


def test_envelope_argument_errors_in_their_order():
    import torch
    from oracle import oracle as O
    last = NO_DEVICE if not torch.cuda.is_available() else None
    u64 = RC._u64
    L = _lib.lib()
    secret = bytes(range(1, 33))
    pub = O.c_public_key(secret)
    env_off = [0, 208, 320, 8624]

    def seal(pubkey=pub, in_off=IN_OFF, lens=LENS, out_off=env_off, d_in=IN, d_out=OUT, scratch=SCR, count=None):
        return L.chipe_seal_ragged_dev(pubkey, len(pubkey) if pubkey else 0, None, d_in, u64(in_off), u64(lens),
                                       len(lens) if count is None else count, d_out, u64(out_off), scratch, None)

    assert seal(count=0) == OK
    assert seal(pubkey=None) == INVALID_ARG and seal(d_out=None) == INVALID_ARG and seal(scratch=None) == INVALID_ARG
    assert seal(in_off=[8, 112, 112, 8320]) == INVALID_ARG and seal(scratch=SCR + 4) == INVALID_ARG
    assert seal(out_off=[0, 100, 320, 8624]) == INVALID_ARG   # envelope 1 (97 bytes, empty object) inside envelope 0
    assert seal(pubkey=b"\x05" * 65) == ECIES and seal(pubkey=pub[:64]) == ECIES
    assert seal(pubkey=b"\x05" * 65, in_off=[8, 112, 112, 8320]) == INVALID_ARG  # INVALID_ARG before ECIES
    if last:
        assert seal() == last and seal(pubkey=O.c_public_key(bytes(range(2, 34)))) == last

    in_len = [n + 97 for n in LENS]
    got = (ctypes.c_uint64 * 4)()

    def open_(sk=secret, in_len=in_len, out_off=IN_OFF, d_in=OUT, d_out=IN, stat=STAT, scratch=SCR, olen=got, count=None):
        return L.chipe_open_ragged_dev(sk, len(sk) if sk else 0, d_in, u64(env_off), u64(in_len),
                                       len(in_len) if count is None else count, d_out, u64(out_off), olen, stat, scratch,
                                       None)

    assert open_(count=0) == OK
    assert open_(sk=None) == INVALID_ARG and open_(stat=None) == INVALID_ARG and open_(olen=None) == INVALID_ARG
    assert open_(d_in=None) == INVALID_ARG and open_(scratch=None) == INVALID_ARG
    assert open_(out_off=[8, 112, 112, 8320]) == INVALID_ARG
    assert open_(sk=bytes(32)) == ECIES and open_(sk=b"\xff" * 32) == ECIES and open_(sk=secret[:31]) == ECIES
    assert open_(sk=bytes(32), out_off=[8, 112, 112, 8320]) == INVALID_ARG      # INVALID_ARG before ECIES
    if last:
        assert open_() == last and list(got) == LENS
        assert open_(in_len=[96, 97, 8290, 113]) == last and list(got) == [0, 0, 8193, 16]  # short: that object's own


def test_one_call_argument_errors_in_their_order():
    import torch
    from oracle import oracle as O
    last = NO_DEVICE if not torch.cuda.is_available() else None
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    secret = bytes(range(1, 33))
    pub = O.c_public_key(secret)
    sizes = [1000, 0, 5000]
    in_off = [0, 1008, 1008]
    env = [n + 97 for n in sizes]
    off = (ctypes.c_uint64 * 3)()
    need = (ctypes.c_uint64 * 3)()
    total = ctypes.c_uint64()
    assert L.chipx_ragged_layout(12, u64(env), 3, 256, 56, off, need, ctypes.byref(total)) == OK
    out_off, got = list(off), (ctypes.c_uint64 * 3)()

    def enc(fmt=13, pubkey=pub, in_off=in_off, sizes=sizes, out_off=out_off, d_hash=STAT, scratch=SCR, count=3):
        return L.chipe_encode_ragged_dev(fmt, pubkey, len(pubkey) if pubkey else 0, None, IN, u64(in_off), u64(sizes),
                                         count, OUT, u64(out_off), got, d_hash, None, scratch, None)

    for fmt in (0, 1, 4, 8, 12, 3, 7, 15, 14, 16, 29):   # no Ecies bit, Ecies alone, the Snappy bit, beyond the bits
        assert enc(fmt=fmt) == INVALID_ARG and enc(fmt=fmt, count=0) == INVALID_ARG
    assert enc(count=0) == OK
    assert enc(pubkey=None) == INVALID_ARG and enc(d_hash=None) == INVALID_ARG and enc(scratch=SCR + 8) == INVALID_ARG
    assert enc(sizes=[1000, 0, (16 << 20) - 96]) == INVALID_ARG           # n + 97 above 16 MiB
    assert enc(out_off=[out_off[0] + 4, out_off[1], out_off[2]]) == INVALID_ARG  # what the ragged encode refuses
    assert enc(in_off=[8, 1008, 1008]) == INVALID_ARG                     # what the envelope seal refuses
    assert enc(pubkey=b"\x05" * 65) == ECIES and enc(pubkey=b"\x05" * 65, in_off=[8, 1008, 1008]) == INVALID_ARG
    if last:
        for fmt in (13, 9, 5):
            assert L.chipx_ragged_layout(fmt & 12, u64(env), 3, 256, 56 if fmt == 13 else 0, off, need,
                                         ctypes.byref(total)) == OK
            assert enc(fmt=fmt, out_off=list(off)) == last and list(got) == list(need)

    in_len = list(need)
    L.chipx_ragged_layout(12, u64(env), 3, 256, 56, off, need, ctypes.byref(total))
    in_len = list(need)

    pads = []
    for e in env:  # the zfec padding of each envelope, as its EncodeInfo would carry it
        pad, chunk = ctypes.c_uint32(), ctypes.c_uint32()
        assert L.chip_calc_padding_len(e, 4, ctypes.byref(pad), ctypes.byref(chunk)) == OK
        pads.append(pad.value)

    def dec(fmt=13, sk=secret, in_len=in_len, out_off=in_off, d_hash=HASH13, stat=STAT, scratch=SCR, count=3):
        return L.chipe_decode_ragged_dev(fmt, sk, len(sk) if sk else 0, OUT, u64(list(off)), u64(in_len), count, d_hash,
                                         u32(pads), IN, u64(out_off), got, stat, scratch, None)

    for fmt in (0, 1, 12, 15, 16):
        assert dec(fmt=fmt) == INVALID_ARG
    assert dec(count=0) == OK
    assert dec(sk=None) == INVALID_ARG and dec(stat=None) == INVALID_ARG and dec(scratch=SCR + 8) == INVALID_ARG
    assert dec(in_len=[in_len[0] + 8, in_len[1], in_len[2]]) == 6       # no bao stream has that length
    assert dec(d_hash=None) == 4                                        # HASH_DECODE
    assert dec(out_off=[8, 1008, 1008]) == INVALID_ARG                  # what the envelope open refuses
    assert dec(sk=bytes(32)) == ECIES and dec(sk=bytes(32), out_off=[8, 1008, 1008]) == INVALID_ARG
    if last:
        assert dec() == last and list(got) == sizes


HASH13 = 0x72000000


def test_scratch_length():
    S = lambda lens: _lib.lib().chipe_gcm_scratch_len(RC._u64(lens), len(lens))  # noqa: E731
    assert S([]) == 0 and _lib.lib().chipe_gcm_scratch_len(None, 3) == 0 and S([(1 << 36) - 31]) == 0
    per_msg = 48 + 96 + 48 + (480 + 2 * 65 * 16 + 32) + 4   # table, header slot, key, key material, verdict
    for lens in ([0], [1], [8192], [8193], [0, 1, 2, 3, 4], [1 << 20] * 7, [(16 << 20) - 97]):
        items = sum(-(-(-(-n // 16)) // 512) for n in lens)
        s = S(lens)
        assert s % 16 == 0 and per_msg * len(lens) + 16 * items <= s <= per_msg * len(lens) + 16 * items + 32, lens
        assert S(lens + [5]) > s and S([n + 8192 for n in lens]) == s + 16 * len(lens)
    # the one-call forms: envelopes, the GCM scratch and the ragged call's scratch
    L = _lib.lib()
    for fmt in (13, 9, 5):
        for lens in ([0], [1000, 0, 5000], [1 << 20] * 3):
            env = [n + 97 for n in lens]
            e = L.chipe_encode_scratch_len(fmt, RC._u64(lens), len(lens))
            want = sum((x + 15) // 16 * 16 for x in env) + S(lens) + L.chipx_ragged_scratch_len(fmt & 12, RC._u64(env),
                                                                                              len(lens), 0)
            assert e % 16 == 0 and want <= e < want + 16
            d = L.chipe_decode_scratch_len(fmt, RC._u64(env), len(env))
            assert d % 16 == 0 and d >= sum(env) + S([max(0, x - 97) for x in env])
    for fmt in (0, 1, 12, 15):
        assert L.chipe_encode_scratch_len(fmt, RC._u64([5]), 1) == 0 == L.chipe_decode_scratch_len(fmt, RC._u64([500]), 1)


@pytest.fixture(scope="module")
def gcm_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "gcm_device_check.cpp", libs=["crypto"])


@pytest.mark.parametrize("args", [["1"], ["0xBEEF"], ["3", "big"]])
def test_gcm_device_and_plan_under_asan_ubsan(gcm_check, args):
    """The text the kernels compile, on the host: S-box circuit against
    FIPS-197 (256 inputs x 32 positions), the C.3 vector, gf128_mul against a
    bit loop, the counter's wrap, byte-granular block moves, the plan, and
    whole messages walked lane by lane as the kernels split them against EVP
    (`big`: the 64-item boundary of the second level, +-1)."""
    assert "0 failures" in B.run_check(gcm_check, *args, timeout=300)


def test_ecies_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "ecies_bench.py"), "--dry-run"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "ecies_bench" and res["dry_run"] is True
    s = res["sets"]
    assert s["1MiB"]["objects"] == 1024 and s["1MiB"]["items"] == 1024 * 128
    assert s["16MiB"]["objects"] == 64 and s["16MiB"]["items"] == 64 * 2048
    assert 200 <= s["tails"]["objects"] <= 256 and all(v["scratch_bytes"] > 0 for v in s.values())
    assert s["1MiB"]["launches"] == {"raw_seal": 3, "raw_open": 4, "env_seal": 4, "env_open": 5}
