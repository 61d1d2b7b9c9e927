"""CPU tests of the snap boundary (include/carbonado_hip_snap.h): the chips_*
symbols beside the seven older sets, their ctypes and Rust bindings, every
error the calls decide before they touch a device, in the header's order, the
scratch and layout lengths, the bench tool's dry run, and the block compressor,
the block decoder, the CRC and the host plan (carbonado_amd/csrc/snap_device.hpp,
snap_plan.hpp) as a stand-alone program under ASan + UBSan against
host_snap.cpp."""
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
HEADER = ROOT / "include" / "carbonado_hip_snap.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_snap.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

OK, INVALID_ARG, HASH_DECODE, BAO_TRUNCATED, ECIES, NO_DEVICE = 0, 1, 4, 6, 17, 100
NAMES = {"chips_abi_version", "chips_snap_scratch_len", "chips_unsnap_scratch_len", "chips_snap_ragged_dev",
         "chips_unsnap_ragged_dev", "chips_encode_layout", "chips_encode_scratch_len", "chips_decode_scratch_len",
         "chips_encode_ragged_dev", "chips_decode_ragged_dev"}
SNAP_FORMATS = (6, 7, 10, 11, 14, 15)


def prototypes() -> dict:
    return B.prototypes(HEADER, "chips_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == 10
    exported = B.exported()
    B.assert_one_set(protos, exported, "chips_")
    assert _lib.lib().chips_abi_version() == 1
    assert "#define CHIPS_ABI_VERSION 1" in HEADER.read_text()
    # the seven older boundaries keep their sets ("chips_" does not start with "chip_")
    B.assert_older_keep_their_sets(exported, "chips_")
    # the argument lists the issue fixes
    assert [n for n, _ in protos["chips_snap_ragged_dev"][1]] == [
        "d_in", "in_off", "n", "count", "d_out", "out_off", "d_out_len", "d_scratch", "scratch_len", "stream"]
    assert [n for n, _ in protos["chips_unsnap_ragged_dev"][1]] == [
        "d_in", "in_off", "in_len", "count", "d_out", "out_off", "out_cap", "d_out_len", "d_status", "d_scratch",
        "scratch_len", "stream"]
    assert [n for n, _ in protos["chips_encode_layout"][1]] == [
        "format", "n", "count", "align", "stream_offset", "out_off", "out_cap", "total"]
    assert [n for n, _ in protos["chips_encode_ragged_dev"][1]] == [
        "format", "pubkey", "pubkey_len", "inject", "d_in", "in_off", "n", "count", "d_out", "out_off", "out_len",
        "d_hash", "info", "d_scratch", "stream"]
    assert [n for n, _ in protos["chips_decode_ragged_dev"][1]] == [
        "format", "secret_key", "sk_len", "d_in", "in_off", "in_len", "count", "d_hash", "padding", "d_out", "out_off",
        "out_cap", "d_out_len", "d_status", "d_scratch", "stream"]


def test_older_entry_points_still_refuse_the_snappy_bit():
    """The eighth header adds; nothing about the Snappy bit changes elsewhere."""
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    got = (ctypes.c_uint64 * 1)()
    for fmt in (2, 3, 6, 7, 10, 11, 14, 15):
        assert L.chipx_encode_ragged_dev(fmt, 0x1000, u64([0]), u64([100]), 1, 0x2000, u64([0]), got, 0x3000, None,
                                         0x4000, None) == INVALID_ARG
        assert L.chipx_decode_ragged_dev(fmt, 0x1000, u64([0]), u64([1096]), 1, 0x3000, u32([0]), 0x2000, u64([0]), got,
                                         0x5000, 0x4000, None) == INVALID_ARG
        assert L.chip_encode_batch_dev(fmt, 0x1000, 1024, 1000, 1, 0x2000, 4096, got, 0x3000, None, 0x4000,
                                       None) == INVALID_ARG
        assert L.chipe_encode_ragged_dev(fmt, b"\x04" * 65, 65, None, 0x1000, u64([0]), u64([100]), 1, 0x2000, u64([0]),
                                         got, 0x3000, None, 0x4000, None) == INVALID_ARG
        assert L.chipe_encode_scratch_len(fmt, u64([100]), 1) == 0


def test_ffi_snap_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chips_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPS_ABI_VERSION: c_int = 1;", text)


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_snap;", lib, flags=re.M)
    for fn, calls in (("snap_scratch", ("chips_snap_scratch_len", "chips_unsnap_scratch_len")),
                      ("snap_ragged", ("chips_snap_ragged_dev",)), ("unsnap_ragged", ("chips_unsnap_ragged_dev",)),
                      ("snap_encode_layout", ("chips_encode_layout",)),
                      ("snap_ragged_scratch", ("chips_encode_scratch_len", "chips_decode_scratch_len")),
                      ("encode_ragged_snap", ("chips_encode_ragged_dev",)),
                      ("decode_ragged_snap", ("chips_decode_ragged_dev",))):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        for call in calls:
            assert f"ffi_snap::{call}(" in body, (fn, call)
    assert "chips_abi_version" in lib


def test_device_module_has_the_bindings():
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    for fn in ("snap_scratch", "snap_ragged", "unsnap_ragged", "snap_encode_layout", "snap_ragged_scratch",
               "encode_ragged_snap", "decode_ragged_snap"):
        assert re.search(rf"^def {fn}\(", src, flags=re.M), fn
    for call in NAMES - {"chips_abi_version"}:
        assert f"{call}(" in src, call


# never dereferenced: the checks come first
IN, OUT, LEN, STAT, SCR, HASH = 0x10000000, 0x40000000, 0x70000000, 0x74000000, 0x78000000, 0x72000000
LENS = [100000, 0, 17, 65536]
IN_OFF = [0, 100000, 100000, 100032]
OUT_OFF = [3, 100200, 100200, 100300]      # any byte address; capacity chip_snap_max_len(n)


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def test_snap_argument_errors_in_their_order():
    u64 = RC._u64
    L = _lib.lib()
    last = _last()
    need = L.chips_snap_scratch_len(u64(LENS), 4)

    def rc(d_in=IN, in_off=IN_OFF, lens=LENS, count=None, d_out=OUT, out_off=OUT_OFF, olen=LEN, scratch=SCR,
           scratch_len=need, arrays=True):
        return L.chips_snap_ragged_dev(d_in, u64(in_off) if arrays else None, u64(lens) if arrays else None,
                                       len(lens) if count is None else count, d_out, u64(out_off) if arrays else None,
                                       olen, scratch, scratch_len, None)

    assert rc(count=0) == OK and rc(count=0, arrays=False, d_in=None, d_out=None, olen=None, scratch=None) == OK
    assert rc(arrays=False) == INVALID_ARG and rc(olen=None) == INVALID_ARG and rc(scratch=None) == INVALID_ARG
    assert rc(count=1 << 31) == INVALID_ARG
    assert rc(lens=[100000, 0, 17, (1 << 40) + 1], scratch_len=1 << 60) == INVALID_ARG
    assert rc(d_in=None) == INVALID_ARG and rc(d_out=None) == INVALID_ARG
    assert rc(in_off=[0, 100000, 100000, (1 << 53) + 16]) == INVALID_ARG
    assert rc(in_off=[8, 100000, 100000, 100032]) == INVALID_ARG and rc(d_in=IN + 4) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    # the worst-case range of object 0 ends at 3 + 10 + 16 + 100000: object 2's stream inside it
    assert rc(out_off=[3, 100200, 100028, 100300]) == INVALID_ARG
    assert rc(scratch_len=need - 1) == INVALID_ARG
    # precedence: a NULL array before the alignment, the alignment before the scratch length
    assert rc(in_off=[8, 100000, 100000, 100032], scratch_len=0) == INVALID_ARG
    if last:
        assert rc() == last
        assert rc(out_off=[3, 100200, 100029, 100300]) == last    # one byte further: no overlap
        assert rc(in_off=[0, 8, 100000, 100032]) == last          # (the empty object's offset is not looked at)
        assert rc(lens=[0, 0, 0, 0], d_in=None, d_out=None) == last


def test_unsnap_argument_errors_in_their_order():
    u64 = RC._u64
    L = _lib.lib()
    last = _last()
    in_len = [5000, 0, 35, 65554]
    in_off = [1, 5001, 5001, 5037]                # any byte address
    cap = [100000, 0, 17, 65536]
    out_off = [0, 100000, 100000, 100032]         # 16-B aligned
    need = L.chips_unsnap_scratch_len(u64(in_len), u64(cap), 4)

    def rc(d_in=IN, in_off=in_off, in_len=in_len, count=None, d_out=OUT, out_off=out_off, cap=cap, olen=LEN, stat=STAT,
           scratch=SCR, scratch_len=need, arrays=True):
        a = (lambda x: u64(x)) if arrays else (lambda x: None)
        return L.chips_unsnap_ragged_dev(d_in, a(in_off), a(in_len), len(in_len) if count is None else count, d_out,
                                         a(out_off), a(cap), olen, stat, scratch, scratch_len, None)

    assert rc(count=0) == OK and rc(count=0, arrays=False, d_in=None, d_out=None, olen=None, stat=None, scratch=None) == OK
    assert rc(arrays=False) == INVALID_ARG and rc(olen=None) == INVALID_ARG and rc(stat=None) == INVALID_ARG
    assert rc(scratch=None) == INVALID_ARG and rc(count=1 << 31) == INVALID_ARG
    assert rc(cap=[100000, 0, 17, (1 << 40) + 1], scratch_len=1 << 60) == INVALID_ARG
    assert rc(d_in=None) == INVALID_ARG and rc(d_out=None) == INVALID_ARG
    assert rc(out_off=[0, 100000, 100000, (1 << 53) + 16]) == INVALID_ARG
    assert rc(out_off=[8, 100000, 100000, 100032]) == INVALID_ARG and rc(d_out=OUT + 4) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    assert rc(out_off=[0, 100000, 99984, 100032]) == INVALID_ARG     # 17 bytes at 99984 end inside object 0's range
    assert rc(scratch_len=need - 1) == INVALID_ARG
    if last:
        assert rc() == last
        assert rc(out_off=[0, 8, 100000, 100032]) == last            # (a zero capacity has no address)
        assert rc(in_len=[0] * 4, d_in=None) == last


def test_one_call_argument_errors_in_their_order():
    from oracle import oracle as O
    last = _last()
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    secret = bytes(range(1, 33))
    pub = O.c_public_key(secret)
    sizes = [1000, 0, 70000]
    in_off = [0, 1008, 1008]
    off, cap, total = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
    got = (ctypes.c_uint64 * 3)()

    def layout(fmt):
        assert L.chips_encode_layout(fmt, u64(sizes), 3, 256, 56 if fmt & 4 else 0, off, cap, ctypes.byref(total)) == OK
        return list(off), list(cap)

    out_off, _ = layout(15)

    def enc(fmt=15, pubkey=pub, in_off=in_off, sizes=sizes, out_off=out_off, d_hash=HASH, scratch=SCR, count=3):
        return L.chips_encode_ragged_dev(fmt, pubkey, len(pubkey) if pubkey else 0, None, IN, u64(in_off), u64(sizes),
                                         count, OUT, u64(out_off), got, d_hash, None, scratch, None)

    for fmt in (0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 30):   # no Snappy bit, Snappy without Bao / Zfec, beyond the bits
        assert enc(fmt=fmt) == INVALID_ARG and enc(fmt=fmt, count=0) == INVALID_ARG
    assert enc(count=0) == OK
    assert enc(pubkey=None) == INVALID_ARG and enc(d_hash=None) == INVALID_ARG and enc(scratch=SCR + 8) == INVALID_ARG
    big = (16 << 20) - 10 - 8 * 256
    assert enc(fmt=14, sizes=[1000, 0, big + 1]) == INVALID_ARG               # worst case above 16 MiB
    assert enc(fmt=15, sizes=[1000, 0, big - 96]) == INVALID_ARG              # ... with the envelope
    assert enc(in_off=[8, 1008, 1008]) == INVALID_ARG                         # what the snap call refuses
    assert enc(out_off=[out_off[0] + 4, out_off[1], out_off[2]]) == INVALID_ARG   # what the ragged encode refuses
    assert enc(out_off=[out_off[0], out_off[1], out_off[0] + 256]) == INVALID_ARG  # worst-case rows that overlap
    assert enc(pubkey=b"\x05" * 65) == ECIES and enc(pubkey=b"\x05" * 65, in_off=[8, 1008, 1008]) == INVALID_ARG
    if last:
        for fmt in SNAP_FORMATS:
            assert enc(fmt=fmt, out_off=layout(fmt)[0]) == last
        assert enc(fmt=14, pubkey=None, out_off=layout(14)[0]) == last   # no key needed without the Ecies bit

    out_off, in_len = layout(14)                     # worst-case lengths are bao stream lengths too
    pads = []
    for n in sizes:
        pad, chunk = ctypes.c_uint32(), ctypes.c_uint32()
        assert L.chip_calc_padding_len(L.chip_snap_max_len(n), 4, ctypes.byref(pad), ctypes.byref(chunk)) == OK
        pads.append(pad.value)

    def dec(fmt=14, sk=None, in_len=in_len, out_off=in_off, caps=sizes, d_hash=HASH, stat=STAT, olen=LEN, scratch=SCR,
            count=3):
        return L.chips_decode_ragged_dev(fmt, sk, len(sk) if sk else 0, OUT, u64(out_off_enc), u64(in_len), count,
                                         d_hash, u32(pads), IN, u64(out_off), u64(caps), olen, stat, scratch, None)

    out_off_enc = out_off
    for fmt in (0, 1, 2, 3, 12, 13, 16):
        assert dec(fmt=fmt) == INVALID_ARG
    assert dec(count=0) == OK
    assert dec(stat=None) == INVALID_ARG and dec(olen=None) == INVALID_ARG and dec(scratch=SCR + 8) == INVALID_ARG
    assert dec(fmt=15) == INVALID_ARG                                        # no secret key with the Ecies bit
    assert dec(in_len=[in_len[0] + 8, in_len[1], in_len[2]]) == BAO_TRUNCATED  # no bao stream has that length
    assert dec(d_hash=None) == HASH_DECODE
    assert dec(out_off=[8, 1008, 1008]) == INVALID_ARG                        # what the unsnap call refuses
    assert dec(in_len=[in_len[0] + 8, in_len[1], in_len[2]], out_off=[8, 1008, 1008]) == BAO_TRUNCATED
    assert dec(fmt=15, sk=bytes(32)) == ECIES and dec(fmt=15, sk=bytes(32), out_off=[8, 1008, 1008]) == INVALID_ARG
    if last:
        assert dec() == last and dec(fmt=15, sk=secret) == last


def test_scratch_and_layout_lengths():
    u64 = RC._u64
    L = _lib.lib()
    S = lambda lens: L.chips_snap_scratch_len(u64(lens), len(lens))            # noqa: E731
    U = lambda lens, caps: L.chips_unsnap_scratch_len(u64(lens), u64(caps), len(lens))  # noqa: E731
    assert S([]) == 0 and L.chips_snap_scratch_len(None, 3) == 0 and S([(1 << 40) + 1]) == 0
    assert U([], []) == 0 and L.chips_unsnap_scratch_len(None, None, 3) == 0 and U([5], [(1 << 40) + 1]) == 0
    slot = (32 + 65536 + 65536 // 6 + 15) // 16 * 16
    for lens in ([0], [1], [65536], [65537], [0, 1, 2, 3, 4], [1 << 20] * 7, [(16 << 20) - 2155]):
        blocks = sum(-(-n // 65536) for n in lens)
        s = S(lens)
        want = 32 * len(lens) + (8 + 16 + slot) * blocks
        assert s % 16 == 0 and want <= s <= want + 48, lens
        more = S([n + 65536 for n in lens]) - s                  # one block more per object (each region rounds to 16)
        assert S(lens + [5]) > s and (16 + slot) * len(lens) <= more <= (8 + 16 + slot) * len(lens) + 16
        slots = blocks + len(lens)
        u = U([n + 100 for n in lens], lens)
        want = (48 + 16) * len(lens) + (4 + 32 + 4) * slots
        assert u % 16 == 0 and want <= u <= want + 64, lens
        assert U([n + 100 for n in lens] + [5], lens + [5]) > u
        assert U([7] * len(lens), lens) == u                   # the capacity sets the slots, not the stream length
    # the layout: chipx_ragged_layout over the worst case
    off, cap, total = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
    xoff, xlen, xtotal = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
    sizes = [1000, 0, 200000]
    for fmt in SNAP_FORMATS:
        worst = [L.chip_snap_max_len(n) + (97 if fmt & 1 else 0) for n in sizes]
        so = 56 if fmt & 4 else 0
        assert L.chips_encode_layout(fmt, u64(sizes), 3, 256, so, off, cap, ctypes.byref(total)) == OK
        assert L.chipx_ragged_layout(fmt & 12, u64(worst), 3, 256, so, xoff, xlen, ctypes.byref(xtotal)) == OK
        assert (list(off), list(cap), total.value) == (list(xoff), list(xlen), xtotal.value)
        e = L.chips_encode_scratch_len(fmt, u64(sizes), 3)
        rows = sum((L.chip_snap_max_len(n) + 15) // 16 * 16 for n in sizes)
        assert e % 16 == 0 and e >= rows + 32 + S(sizes)
        assert L.chips_encode_scratch_len(fmt, u64(sizes + [5]), 4) > e
        d = L.chips_decode_scratch_len(fmt, cap, u64(sizes), 3)
        assert d % 16 == 0 and d >= sum(cap) + U(list(cap), sizes)
    for fmt in (0, 1, 2, 3, 4, 12, 13, 16):
        assert L.chips_encode_layout(fmt, u64(sizes), 3, 256, 0, off, cap, ctypes.byref(total)) == INVALID_ARG
        assert L.chips_encode_scratch_len(fmt, u64([5]), 1) == 0
        assert L.chips_decode_scratch_len(fmt, u64([500]), u64([5]), 1) == 0
    assert L.chips_encode_layout(14, u64([(16 << 20)]), 1, 256, 56, off, cap, ctypes.byref(total)) == INVALID_ARG
    assert L.chips_encode_scratch_len(14, u64([(16 << 20)]), 1) == 0


@pytest.fixture(scope="module")
def snap_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "snap_device_check.cpp",
                         extra_sources=[ROOT / "carbonado_amd" / "csrc" / "host_snap.cpp"])


@pytest.mark.parametrize("args", [["1"], ["0xBEEF"], ["3", "big"]])
def test_snap_device_and_plan_under_asan_ubsan(snap_check, args):
    """The text the kernels compile, on the host: the CRC segment-and-combine
    against crc_masked at every length 0..130 and at 65535 / 65536, objects
    compressed as the kernels split them against host::snap_compress byte for
    byte, the block decoder against host::decompress_raw on good and corrupt
    bodies, and the plan."""
    assert "0 failures" in B.run_check(snap_check, *args, timeout=300)


def test_snap_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "snap_bench.py"), "--dry"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "snap_bench" and res["dry_run"] is True
    s = res["sets"]
    assert s["1MiB"]["objects"] == 1024 and s["1MiB"]["blocks"] == 1024 * 16 and s["1MiB"]["slots"] == 1024 * 17
    assert s["16MiB"]["objects"] == 64 and s["16MiB"]["blocks"] == 64 * 256 and s["16MiB"]["slots"] == 64 * 257
    assert all(v["snap_scratch_bytes"] > v["object_bytes"] and v["unsnap_scratch_bytes"] > 0 for v in s.values())
    assert s["1MiB"]["launches"] == {"raw_snap": 3, "raw_unsnap": 4}
