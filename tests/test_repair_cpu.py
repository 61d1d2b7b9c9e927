"""CPU tests of the repair boundary (include/carbonado_hip_repair.h): the
chipr_* symbols, their ctypes and Rust bindings, the argument errors a ragged
scrub decides before it touches a device, in their stated order, the scratch
length, and the host logic behind them (carbonado_amd/csrc/repair_plan.hpp)
as a stand-alone program under ASan + UBSan."""
import ctypes
import re
from pathlib import Path

import pytest

import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
REPAIR_HEADER = ROOT / "include" / "carbonado_hip_repair.h"
FFI_REPAIR = ROOT / "carbonado-hip" / "src" / "ffi_repair.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

OK, INVALID_ARG, HASH_DECODE, TRUNCATED, NO_DEVICE = 0, 1, 4, 6, 100


def repair_prototypes() -> dict:
    return B.prototypes(REPAIR_HEADER, "chipr_")


def test_repair_exports_header_and_ctypes_are_one_set():
    protos = repair_prototypes()
    assert len(protos) == 4
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipr_")
    assert _lib.lib().chipr_abi_version() == 1
    assert "#define CHIPR_ABI_VERSION 1" in REPAIR_HEADER.read_text()
    # the three older boundaries keep their sets
    B.assert_older_keep_their_sets(exported, "chipr_")


def test_ffi_repair_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI_REPAIR, "chipr_"), repair_prototypes())
    text = B.ffi_text(FFI_REPAIR)
    assert re.search(r"pub const CHIPR_ABI_VERSION: c_int = 1;", text)


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_repair;", lib, flags=re.M)
    for fn, call in (("shard_masks_ragged", "chipr_shard_masks_ragged_dev"), ("scrub_ragged", "chipr_scrub_ragged_dev"),
                     ("scrub_ragged_scratch_len", "chipr_scrub_ragged_scratch_len")):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert f"ffi_repair::{call}(" in body, fn
    for fn in ("shard_masks_ragged", "scrub_ragged"):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert "DeviceBuffer" in lib[m.end():].split("{", 1)[0]


def _u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs)


def _u32(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def _blen(n):
    return 8 + n + 64 * (max(1, -(-n // 1024)) - 1)


# never dereferenced: the checks come first
STR, OUT, HASH, MASKS, SCR = 0x10000000, 0x40000000, 0x70000000, 0x74000000, 0x78000000
SPC = [1, 5, 9]
LEN3 = [_blen(8192 * s) for s in SPC]
OFF3 = [56, 1 << 20, (2 << 20) + 8]
CL3 = [1024 * s for s in SPC]
PAD3 = [38, 42, 46]


def _need(in_len=LEN3, nrepair=1):
    return _lib.lib().chipr_scrub_ragged_scratch_len(_u64(in_len), len(in_len), nrepair)


def _scrub(in_off=OFF3, in_len=LEN3, out_off=OFF3, enc=STR, out=OUT, hashes=HASH, scratch=SCR, scratch_len=None,
           count=None, arrays=True, status=True):
    count = len(in_len) if count is None else count
    st = (ctypes.c_int32 * 3)()
    scratch_len = _need(in_len) if scratch_len is None else scratch_len
    return _lib.lib().chipr_scrub_ragged_dev(enc, _u64(in_off), _u64(in_len) if arrays else None, count, hashes,
                                             _u32(PAD3), _u32(CL3), out, _u64(out_off), st if status else None, scratch,
                                             scratch_len, None)


def _masks(in_off=OFF3, in_len=LEN3, enc=STR, hashes=HASH, masks=MASKS, scratch=SCR, scratch_len=None, count=None,
           arrays=True):
    count = len(in_len) if count is None else count
    scratch_len = _need(in_len) if scratch_len is None else scratch_len
    return _lib.lib().chipr_shard_masks_ragged_dev(enc, _u64(in_off), _u64(in_len), count, hashes,
                                                   _u32(CL3) if arrays else None, masks, scratch, scratch_len, None)


def test_repair_argument_errors_need_no_device():
    # NULL arrays or buffers with count > 0
    assert _scrub(arrays=False) == INVALID_ARG and _masks(arrays=False) == INVALID_ARG
    assert _scrub(enc=None) == INVALID_ARG and _scrub(out=None) == INVALID_ARG and _scrub(status=False) == INVALID_ARG
    assert _scrub(scratch=None) == INVALID_ARG and _masks(masks=None) == INVALID_ARG and _masks(enc=None) == INVALID_ARG
    assert _scrub(count=1 << 31) == INVALID_ARG and _masks(count=1 << 31) == INVALID_ARG
    # stream and output addresses want 8, the scratch 16
    assert _scrub(in_off=[60, OFF3[1], OFF3[2]]) == INVALID_ARG and _masks(in_off=[56, OFF3[1] + 4, OFF3[2]]) == INVALID_ARG
    assert _scrub(out_off=[56, OFF3[1], OFF3[2] + 4]) == INVALID_ARG
    assert _scrub(scratch=SCR + 8) == INVALID_ARG and _masks(scratch=SCR + 8) == INVALID_ARG
    # overlaps: two outputs (either order); an output over part of an input; in place is fine
    assert _scrub(out_off=[56, 56 + LEN3[0] - 8, OFF3[2]]) == INVALID_ARG
    assert _scrub(out_off=[56 + LEN3[1] - 8, 56, OFF3[2]]) == INVALID_ARG
    assert _scrub(out=STR, out_off=[56 + 8, 4 << 20, 6 << 20]) == INVALID_ARG  # over part of its own input
    assert _scrub(out=STR, out_off=[4 << 20, 56, 6 << 20]) == INVALID_ARG      # over another object's input
    assert _scrub(out=STR, out_off=[4 << 20, OFF3[1] + LEN3[1] - 8, 6 << 20]) == INVALID_ARG
    # a stream of more than 32 MiB of content
    assert _scrub(in_len=[LEN3[0], _blen((32 << 20) + 8192), LEN3[2]], out_off=[56, 1 << 20, 40 << 20],
                  in_off=[56, 1 << 20, 40 << 20], scratch_len=1 << 40) == INVALID_ARG
    assert _scrub(in_len=[LEN3[0], _blen(32 << 20), LEN3[2]], out_off=[56, 1 << 20, 40 << 20],
                  in_off=[56, 1 << 20, 40 << 20], hashes=None) == HASH_DECODE
    # a scratch one byte short
    assert _scrub(scratch_len=_need() - 1) == INVALID_ARG and _masks(scratch_len=_need() - 1) == INVALID_ARG
    # no bao stream has that length
    gap = [LEN3[0], LEN3[1] + 8, LEN3[2]]
    assert _scrub(in_len=gap) == TRUNCATED and _masks(in_len=gap) == TRUNCATED
    assert _scrub(in_len=[7, LEN3[1], LEN3[2]]) == TRUNCATED
    # INVALID_ARG before BAO_TRUNCATED before HASH_DECODE
    assert _scrub(in_len=gap, out_off=[56, OFF3[1], OFF3[2] + 4]) == INVALID_ARG
    assert _scrub(in_len=gap, scratch_len=_need(gap) - 1) == INVALID_ARG
    assert _scrub(hashes=None) == HASH_DECODE and _masks(hashes=None) == HASH_DECODE
    assert _scrub(hashes=None, in_len=gap) == TRUNCATED and _masks(hashes=None, in_len=gap) == TRUNCATED
    # nothing to do
    assert _scrub(count=0) == OK and _masks(count=0) == OK
    assert _scrub(count=0, arrays=False, enc=None, out=None, hashes=None, scratch=None, status=False) == OK
    # a well-formed call, also in place, gets as far as the device and no further
    import torch
    if not torch.cuda.is_available():
        assert _scrub() == NO_DEVICE and _masks() == NO_DEVICE
        assert _scrub(out=STR) == NO_DEVICE  # every output range exactly its own input range
        assert _scrub(out=STR, out_off=[OFF3[0], 4 << 20, OFF3[2]]) == NO_DEVICE  # in place for two, elsewhere for one


def test_scrub_ragged_scratch_len_is_monotone_and_clamps():
    spcs = (1, 64, 3, 512, 9, 64, 2)
    lens = [_blen(8192 * s) for s in spcs]
    got = [_need(lens, r) for r in range(0, len(lens) + 3)]
    assert got[0] == got[1]                                # nrepair clamped to 1 from below
    assert all(a <= b for a, b in zip(got, got[1:]))       # monotone
    assert got[len(lens)] == got[len(lens) + 1] == got[len(lens) + 2]  # and to count from above
    assert got[1] < got[2] < got[len(lens)] and all(g % 16 == 0 for g in got)
    # one pass of r repairs holds the r largest streams: primaries (half the content) and a staged row each
    big = sorted(spcs, reverse=True)
    for r in (1, 2, len(lens)):
        floor = sum(_blen(8192 * s) + 4096 * s for s in big[:r])
        assert floor <= got[r] <= floor + 64 * 1024
    # lengths a call would reject count as empty; no streams at all
    assert _need([LEN3[0] + 8, 7], 2) == _need([0, 0], 2) and _need([], 1) % 16 == 0


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "repair_plan_check.cpp")


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_repair_plan_under_asan_ubsan(plan_check, seed):
    """Checks, scratch layout, verdict requests, passes and records of a ragged
    scrub are host code (repair_plan.hpp): a stand-alone program drives them
    over seeded mixes (disjoint scratch regions inside the reported length,
    every repair in exactly one pass) and multiplies the record's coefficients
    with the selected rows of the encoding matrix for all 70 four-subsets."""
    assert "0 failures" in B.run_check(plan_check, seed)
