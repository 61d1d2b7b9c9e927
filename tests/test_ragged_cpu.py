"""CPU tests of the extension boundary (include/carbonado_hip_ext.h): the
chipx_* symbols, their ctypes and Rust bindings, the host-only layout helper
against the oracle, the argument errors a ragged call decides before it
touches a device, and the host logic behind them under ASan + UBSan."""
import ctypes
import re
from pathlib import Path

import pytest

import test_abi
import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
EXT_HEADER = ROOT / "include" / "carbonado_hip_ext.h"
FFI_EXT = ROOT / "carbonado-hip" / "src" / "ffi_ext.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3072, 4095, 4096, 4097, 8192,
         32768, 32769, 65535, 65536, 65537, 66560, 131073, 200001, 262144, 266240,
         1 << 20, (1 << 20) + 5]
OK, INVALID_ARG, UNEVEN = 0, 1, 3


def ext_prototypes() -> dict:
    return B.prototypes(EXT_HEADER, "chipx_")


def test_ext_exports_header_and_ctypes_are_one_set():
    protos = ext_prototypes()
    assert len(protos) == 5
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipx_")
    L = _lib.lib()
    assert L.chipx_abi_version() == 1
    assert "#define CHIPX_ABI_VERSION 1" in EXT_HEADER.read_text()


def test_drop_in_boundary_is_unchanged():
    L = _lib.lib()
    assert L.chip_abi_version() == 5
    exported = B.exported()
    chip = B.exports_of(exported, "chip_")
    assert chip == test_abi.header_symbols() == set(_lib.SIGNATURES)
    B.assert_older_keep_their_sets(exported, "chipx_")


def test_ffi_ext_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI_EXT, "chipx_"), ext_prototypes())
    text = B.ffi_text(FFI_EXT)
    assert re.search(r"pub const CHIPX_ABI_VERSION: c_int = 1;", text)


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_ext;", lib, flags=re.M)
    for fn, call in (("encode_ragged", "chipx_encode_ragged_dev"), ("decode_ragged", "chipx_decode_ragged_dev")):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert f"ffi_ext::{call}(" in body, fn
        assert "DeviceBuffer" in body.split("{", 1)[0]
    assert (ROOT / "carbonado-hip" / "src" / "ffi.rs").exists()


def _u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs)


@pytest.mark.parametrize("level", [4, 8, 12])
@pytest.mark.parametrize("stream_offset", [0, 56])
def test_ragged_layout_matches_oracle(level, stream_offset):
    L = _lib.lib()
    off, ln, total = _u64([0] * len(SIZES)), _u64([0] * len(SIZES)), ctypes.c_uint64()
    assert L.chipx_ragged_layout(level, _u64(SIZES), len(SIZES), 256, stream_offset, off, ln,
                                 ctypes.byref(total)) == OK
    rows = []
    for i, n in enumerate(SIZES):
        assert ln[i] == len(O.encode(bytes(n), level)[0]), (level, n)
        if level & 4:
            assert off[i] % 256 == stream_offset
        else:
            assert off[i] % 16 == 0
        rows.append((off[i], off[i] + ln[i]))
    rows.sort()
    assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:])), "rows overlap"
    assert total.value >= rows[-1][1] and total.value % 256 == 0
    assert L.chipx_ragged_layout(level, _u64(SIZES), len(SIZES), 100, 0, off, ln, ctypes.byref(total)) == INVALID_ARG
    assert L.chipx_ragged_layout(15, _u64(SIZES), len(SIZES), 256, 0, off, ln, ctypes.byref(total)) == INVALID_ARG


IN, OUT, HASH, SCR = 0x10000000, 0x40000000, 0x70000000, 0x78000000  # never dereferenced: the checks come first


def _encode(level, in_off, n, out_off, count=None):
    count = len(n) if count is None else count
    return _lib.lib().chipx_encode_ragged_dev(level, IN, _u64(in_off), _u64(n), count, OUT, _u64(out_off),
                                              _u64([0] * len(n)), HASH, None, SCR, None)


def _decode(level, in_off, in_len, out_off, padding=None, count=None):
    count = len(in_len) if count is None else count
    pads = (ctypes.c_uint32 * max(len(in_len), 1))(*(padding or [0] * len(in_len)))
    return _lib.lib().chipx_decode_ragged_dev(level, IN, _u64(in_off), _u64(in_len), count, HASH, pads, OUT,
                                              _u64(out_off), _u64([0] * len(in_len)), SCR, SCR, None)


@pytest.mark.parametrize("level", [4, 8, 12])
def test_ragged_argument_errors_need_no_device(level):
    n, in_off, out_off = [5000, 70000], [0, 8192], [0, 1 << 20]
    for bad in (level | 1, level | 2, 0, 16 | level):  # Ecies, Snappy, no device stage, not a format
        assert _encode(bad, in_off, n, out_off) == INVALID_ARG
        assert _decode(bad, in_off, [8200, 8200], out_off) == INVALID_ARG
    assert _encode(level, [0, 8200], n, out_off) == INVALID_ARG          # input at 8 mod 16
    assert _encode(level, in_off, n, [0, (1 << 20) + 4]) == INVALID_ARG   # output at 4 mod 8
    if level == 8:
        assert _encode(level, in_off, n, [0, (1 << 20) + 8]) == INVALID_ARG  # shards want 16
    assert _encode(level, in_off, n, [0, 4096]) == INVALID_ARG            # outputs overlap
    assert _encode(level, in_off, n, [4096, 0]) == INVALID_ARG            # in either order
    assert _encode(level, in_off, [5000, (16 << 20) + 1], out_off) == INVALID_ARG
    assert _encode(level, in_off, n, out_off, count=0) == OK
    assert _decode(level, in_off, [8, 8], out_off, count=0) == OK
    enc = [len(O.encode(bytes(x), level)[0]) for x in n]
    pad = [(-x) % 4096 if level & 8 else 0 for x in n]
    eoff = [0, 1 << 20]
    assert _decode(level, [0, (1 << 20) + 4], enc, [0, 1 << 20], pad) == INVALID_ARG  # input at 4 mod 8
    assert _decode(level, eoff, enc, [0, (1 << 20) + 8], pad) == INVALID_ARG           # output at 8 mod 16
    assert _decode(level, eoff, enc, [0, 16], pad) == INVALID_ARG                      # outputs overlap
    if level == 8:
        assert _decode(level, eoff, [enc[0], enc[1] + 4], [0, 1 << 20], pad) == UNEVEN
        assert _decode(level, eoff, [enc[0], (32 << 20) + 8], [0, 1 << 20], pad) == INVALID_ARG  # oversize
    if level == 12:
        assert _decode(level, eoff, [enc[0], enc[1] + 1], [0, 1 << 20], pad) == 6  # no bao stream has that length
    # a valid call gets as far as the device and no further
    import torch
    if not torch.cuda.is_available():
        assert _encode(level, in_off, n, out_off) == 100
        assert _decode(level, eoff, enc, [0, 1 << 20], pad) == 100


def test_ragged_scratch_len_covers_the_tables():
    L = _lib.lib()
    for level in (4, 8, 12):
        small = L.chipx_ragged_scratch_len(level, _u64(SIZES), len(SIZES), 0)
        assert small >= 64 * len(SIZES) + 8 * (len(SIZES) + 1)
        groups = sum(max(1, -(-len(O.encode(bytes(n), level & 8)[0]) // 65536)) for n in SIZES) if level & 4 else 0
        assert small >= 64 * len(SIZES) + 8 * (len(SIZES) + 1) + 32 * groups
        assert small < (1 << 16)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "ragged_plan_check.cpp")


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_ragged_plan_under_asan_ubsan(plan_check, seed):
    """The descriptor / layout / overlap logic of a ragged call is host code
    (ragged_plan.hpp): a stand-alone program drives it over seeded mixes."""
    assert "0 failures" in B.run_check(plan_check, seed)
