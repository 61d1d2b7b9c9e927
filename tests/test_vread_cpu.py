"""CPU tests of the vouched-read boundary (include/carbonado_hip_vread.h): the
chipv_* symbols, their ctypes and Rust bindings, the argument errors a vouched
read decides before it touches a device, in their stated order, the scratch
length, and the host logic behind them (carbonado_amd/csrc/vread_plan.hpp) as
a stand-alone program under ASan + UBSan."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

import test_read_cpu as RC
import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
VREAD_HEADER = ROOT / "include" / "carbonado_hip_vread.h"
FFI_VREAD = ROOT / "carbonado-hip" / "src" / "ffi_vread.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

OK, INVALID_ARG, HASH_DECODE, TRUNCATED, NO_DEVICE = 0, 1, 4, 6, 100
STRICT = 1


def vread_prototypes() -> dict:
    return B.prototypes(VREAD_HEADER, "chipv_")


def test_vread_exports_header_and_ctypes_are_one_set():
    protos = vread_prototypes()
    assert set(protos) == {"chipv_abi_version", "chipv_read_scratch_len", "chipv_read_ranges_dev"}
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipv_")
    assert _lib.lib().chipv_abi_version() == 1
    text = VREAD_HEADER.read_text()
    assert "#define CHIPV_ABI_VERSION 1" in text and "#define CHIPV_STRICT 1u" in text
    # the argument list of chipd_read_ranges_dev plus d_vouch behind d_used and flags in front of d_scratch
    old = [n for n, _ in RC.read_prototypes()["chipd_read_ranges_dev"][1]]
    new = [n for n, _ in protos["chipv_read_ranges_dev"][1]]
    assert new == old[:old.index("d_used") + 1] + ["d_vouch", "flags"] + old[old.index("d_scratch"):]
    types = dict(protos["chipv_read_ranges_dev"][1])
    assert types["d_vouch"] == "*mut u32" and types["flags"] == "u32"
    # the five older boundaries keep their sets
    B.assert_older_keep_their_sets(exported, "chipv_")
    # the ctypes of the new call: those of the old one with the two arguments put in
    o, n = _lib.READ_SIGNATURES["chipd_read_ranges_dev"][1], _lib.VREAD_SIGNATURES["chipv_read_ranges_dev"][1]
    assert n == o[:16] + [ctypes.c_void_p, ctypes.c_uint32] + o[16:]


def test_ffi_vread_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI_VREAD, "chipv_"), vread_prototypes())
    text = B.ffi_text(FFI_VREAD)
    assert re.search(r"pub const CHIPV_ABI_VERSION: c_int = 1;", text)
    header = VREAD_HEADER.read_text()
    for name in ("CHIPV_VOUCHED", "CHIPV_UNVOUCHED", "CHIPV_CONTRADICTED", "CHIPV_STRICT"):
        c = re.search(rf"#define {name} (\d+)u", header).group(1)
        assert re.search(rf"pub const {name}: u32 = {c};", text), name


def test_lib_rs_has_the_safe_wrapper():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_vread;", lib, flags=re.M)
    for fn, call in (("vread_scratch_len", "chipv_read_scratch_len"), ("read_ranges_vouched", "chipv_read_ranges_dev")):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert f"ffi_vread::{call}(" in body, fn
    m = re.search(r"\npub fn read_ranges_vouched\(", lib)
    sig = lib[m.end():].split("{", 1)[0]
    assert "DeviceBuffer" in sig and "vouch: &mut DeviceBuffer" in sig and "flags: u32" in sig
    assert "chipv_abi_version" in lib


def test_device_module_has_the_bindings():
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^def vread_scratch\(", src, flags=re.M) and re.search(r"^def read_ranges_vouched\(", src, flags=re.M)
    assert "chipv_read_ranges_dev(" in src and "chipv_read_scratch_len(" in src


STR, OUT, HASH, STAT, USED, SCR = RC.STR, RC.OUT, RC.HASH, RC.STAT, RC.USED, RC.SCR
VOUCH = 0x77000000


def _need(nreq=4, nseg=RC.NSEG4):
    return _lib.lib().chipv_read_scratch_len(nreq, nseg)


def _vread(in_off=RC.OFF3, in_len=RC.LEN3, rs=RC.RS4, start=RC.ST4, length=RC.LN4, co=RC.CO4, enc=STR, out=OUT,
           hashes=HASH, stat=STAT, used=USED, vouch=VOUCH, flags=0, scratch=SCR, scratch_len=None, nreq=None, arrays=True,
           clen=True, chunk_len=RC.CL3):
    nreq = len(rs) if nreq is None else nreq
    got = (ctypes.c_uint64 * 8)()
    scratch_len = _need() if scratch_len is None else scratch_len
    u64, u32 = RC._u64, RC._u32
    rc = _lib.lib().chipv_read_ranges_dev(enc, u64(in_off), u64(in_len) if arrays else None, hashes, u32(RC.PAD3),
                                          u32(chunk_len), len(in_len), u32(rs), u64(start), u64(length), nreq, out,
                                          u64(co), got if clen else None, stat, used, vouch, flags, scratch, scratch_len,
                                          None)
    return rc, list(got)[:4]


def test_vread_argument_errors_need_no_device():
    import torch
    last = NO_DEVICE if not torch.cuda.is_available() else None
    OFF3, LEN3, CO4 = RC.OFF3, RC.LEN3, RC.CO4

    def rc(**kw):
        return _vread(**kw)[0]
    # NULL arrays or buffers with nreq > 0, d_vouch among them
    assert rc(arrays=False) == INVALID_ARG and rc(clen=False) == INVALID_ARG and rc(enc=None) == INVALID_ARG
    assert rc(out=None) == INVALID_ARG and rc(stat=None) == INVALID_ARG and rc(used=None) == INVALID_ARG
    assert rc(vouch=None) == INVALID_ARG and rc(scratch=None) == INVALID_ARG
    # a flag bit other than CHIPV_STRICT
    for f in (2, 4, 3, 1 << 31, 0xFFFFFFFE):
        assert rc(flags=f) == INVALID_ARG
    assert rc(nreq=1 << 31) == INVALID_ARG
    # a request of a stream that is not there; a start or len above 2^53
    assert rc(rs=[0, 1, 3, 2]) == INVALID_ARG
    assert rc(start=[100, (1 << 53) + 1, 5, 7]) == INVALID_ARG and rc(length=[50, 1, (1 << 53) + 1, 0]) == INVALID_ARG
    # stream addresses want 8, content addresses and the scratch 16
    assert rc(in_off=[60, OFF3[1], OFF3[2]]) == INVALID_ARG and rc(in_off=[56, OFF3[1] + 4, OFF3[2]]) == INVALID_ARG
    assert rc(co=[0, 72, CO4[2], CO4[3]]) == INVALID_ARG and rc(out=OUT + 8) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    # two content ranges that overlap (either order); an empty range overlaps nothing
    assert rc(co=[0, 48, CO4[2], CO4[3]]) == INVALID_ARG and rc(co=[CO4[2], 64, 48 + 20448, CO4[3]]) == INVALID_ARG
    if last:
        assert rc(co=[0, 64, CO4[2], 0]) == last
    # a scratch one byte short; the scratch of the unvouched call is too short as well
    assert rc(scratch_len=_need() - 1) == INVALID_ARG
    assert rc(scratch_len=RC._need()) == INVALID_ARG
    # no bao stream has that length
    gap = [LEN3[0], LEN3[1] + 8, LEN3[2]]
    assert rc(in_len=gap) == TRUNCATED and rc(in_len=[7, LEN3[1], LEN3[2]]) == TRUNCATED
    # INVALID_ARG before BAO_TRUNCATED before HASH_DECODE
    assert rc(in_len=gap, co=[0, 72, CO4[2], CO4[3]]) == INVALID_ARG
    assert rc(in_len=gap, scratch=SCR + 8) == INVALID_ARG
    assert rc(in_len=gap, flags=2) == INVALID_ARG and rc(hashes=None, flags=8) == INVALID_ARG
    assert rc(in_len=gap, scratch_len=_need(4, 3) - 1) == INVALID_ARG  # (the misfit stream's request has no segment)
    assert rc(hashes=None) == HASH_DECODE and rc(hashes=None, in_len=gap) == TRUNCATED
    assert rc(hashes=None, scratch_len=_need() - 1) == INVALID_ARG
    # nothing to do, whatever the flags
    assert rc(nreq=0) == OK and rc(nreq=0, flags=0xFF) == OK
    assert rc(nreq=0, arrays=False, enc=None, out=None, hashes=None, scratch=None, stat=None, used=None, vouch=None,
              clen=False) == OK
    # a well-formed call gets as far as the device and no further; the lengths are written before that
    if last:
        for f in (0, STRICT):
            code, got = _vread(flags=f)
            assert code == last and got == [50, 4 * RC.CL3[1] - RC.PAD3[1], 10, 0]
        code, got = _vread(chunk_len=[1024, 5120 + 1024, 9216], scratch_len=_need(4, 3))
        assert code == last and got == [50, 0, 10, 0]


def test_vread_scratch_length():
    S, D = _lib.lib().chipv_read_scratch_len, _lib.lib().chipd_read_scratch_len
    grid = [(a, b) for a in (0, 1, 2, 77, 1000, 4097) for b in (0, 1, 3, 64, 65, 300, 4000, 1 << 20)]
    for a, b in grid:
        assert S(a, b) % 16 == 0 and S(a, b) >= D(a, b), (a, b)
        assert S(a + 1, b) >= S(a, b) and S(a, b + 1) >= S(a, b), (a, b)
    assert S(10, 10) <= S(11, 10) <= S(11, 40) and S(1000, 4000) > S(10, 40)
    # two words per segment more than the unvouched call
    assert S(1000, 1 << 20) - D(1000, 1 << 20) >= 8 << 20


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "vread_plan_check.cpp")


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_vread_plan_under_asan_ubsan(plan_check, seed):
    """The extra checks, the scratch layout and the vouch items of a vouched
    read are host code (vread_plan.hpp): a stand-alone program drives them over
    seeded mixes (the plan is a ranged read's plan, the scratch regions are
    disjoint inside the reported length, the vouch items of a segment are its
    window's chunks and every item maps back to (segment, chunk) once)."""
    assert "0 failures" in B.run_check(plan_check, seed)


def test_vread_bench_dry_run():
    """tools/vread_bench.py lays its three request sets out without a device."""
    import json
    import sys
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "vread_bench.py"), "--dry-run", "--streams", "128"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "vread_bench" and res["dry_run"] is True
    assert res["intact"]["requests"] == 128 and res["sixteen_per_stream"]["requests"] == 2048
    assert res["damaged_1_in_64"]["damaged"] == 2
    for case in ("intact", "damaged_1_in_64", "sixteen_per_stream"):
        c = res[case]
        assert c["requests"] <= c["segments"] <= 2 * c["requests"]
        assert c["scratch_bytes"] >= c["scratch_bytes_unvouched"] + 8 * c["segments"]
