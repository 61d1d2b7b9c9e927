"""CPU tests of the qread boundary (include/carbonado_hip_qread.h): the chipq_*
symbols beside the ten older sets, their ctypes and Rust bindings, the errors
the calls decide before they touch a device, in the header's order, the table
and scratch lengths, the bench tool's dry run, and the planning text the
request kernel compiles (carbonado_amd/csrc/qread_device.hpp) with the host's
O(1) share (qread_plan.hpp) as a stand-alone program under ASan + UBSan."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

import boundary as B
import test_read_cpu as RC
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "carbonado_hip_qread.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_qread.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"
CSRC = ROOT / "carbonado_amd" / "csrc"

OK, INVALID_ARG, HASH_DECODE, TRUNCATED, NO_DEVICE = 0, 1, 4, 6, 100
NAMES = {"chipq_abi_version", "chipq_stream_table_len", "chipq_stream_table_dev", "chipq_read_scratch_len",
         "chipq_read_ranges_dev", "chipq_read_ranges_vouched_dev"}
# the eleventh boundary; boundary.BOUNDARIES holds the first nine, test_fread_cpu the tenth
MINE = B._boundary("chipq_", "qread", _lib.QREAD_SIGNATURES, 6)
OLDER = B.BOUNDARIES + (B._boundary("chipf_", "fread", _lib.FREAD_SIGNATURES, 7),)


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipq_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == MINE.exports
    exported = B.exported()
    assert set(protos) == B.exports_of(exported, MINE.prefix) == set(MINE.signatures)
    for name, (_, ps) in protos.items():
        assert len(MINE.signatures[name][1]) == len(ps), name
    assert _lib.lib().chipq_abi_version() == 1
    assert "#define CHIPQ_ABI_VERSION 1" in HEADER.read_text()
    # every older boundary keeps its count; no prefix clashes, no shared name
    assert [b.exports for b in OLDER] == [62, 5, 6, 4, 4, 3, 10, 10, 8, 7]
    for b in OLDER:
        assert len(B.exports_of(exported, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(MINE.prefix) and not MINE.prefix.startswith(b.prefix)
        assert not set(MINE.signatures) & set(b.signatures), b.prefix
    # the argument lists the header states
    streams = ["d_streams", "in_off", "in_len", "d_hash", "padding", "chunk_len", "nstreams"]
    assert [n for n, _ in protos["chipq_stream_table_dev"][1]] == streams + ["d_table", "table_len", "info", "stream"]
    assert [n for n, _ in protos["chipq_read_scratch_len"][1]] == ["info", "nreq", "max_len", "vouched"]
    read = ["d_table", "info", "d_req_stream", "d_start", "d_len", "nreq", "max_len", "d_content", "content_stride",
            "d_content_len", "d_status", "d_used", "d_scratch", "scratch_len", "stream"]
    assert [n for n, _ in protos["chipq_read_ranges_dev"][1]] == read
    assert [n for n, _ in protos["chipq_read_ranges_vouched_dev"][1]] == read[:12] + ["d_vouch", "flags"] + read[12:]
    assert ctypes.sizeof(_lib.TableInfo) == 32


def test_ffi_qread_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipq_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPQ_ABI_VERSION: c_int = 1;", text)
    m = re.search(r"#\[repr\(C\)\][^{]*pub struct chipq_table_info \{([^}]*)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+): (\w+)", m.group(1)) == [("nstreams", "u64"), ("max_chunks", "u64"),
                                                          ("min_shard", "u64"), ("reserved", "u64")]
    header = RS._strip_comments(HEADER.read_text())
    body = re.search(r"typedef struct chipq_table_info \{([^}]*)\}", header, flags=re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", body) == ["nstreams", "max_chunks", "min_shard", "reserved"]


WRAPPERS = (("stream_table_len", "stream_table", ("chipq_stream_table_len",)),
            ("stream_table", "stream_table", ("chipq_stream_table_dev",)),
            ("planned_read_scratch_len", "planned_read_scratch", ("chipq_read_scratch_len",)),
            ("read_ranges_planned", "read_ranges_planned", ("chipq_read_ranges_dev",)),
            ("read_ranges_vouched_planned", "read_ranges_vouched_planned", ("chipq_read_ranges_vouched_dev",)))


def test_lib_rs_and_device_module_have_the_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^mod ffi_qread;", lib, flags=re.M) and "chipq_abi_version" in lib
    for rust_fn, py_fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {rust_fn}\(", lib)
        assert m, rust_fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert re.search(rf"^def {py_fn}\(", src, flags=re.M), py_fn
        for call in calls:
            assert f"ffi_qread::{call}(" in body, (rust_fn, call)
            assert f"{call}(" in src, call


# never dereferenced: the checks come first
STR, OUT, HASH, STAT, USED, SCR = RC.STR, RC.OUT, RC.HASH, RC.STAT, RC.USED, RC.SCR
TAB, REQ, START, LEN, CLEN, VOUCH = 0x79000000, 0x7A000000, 0x7A100000, 0x7A200000, 0x7A300000, 0x77000000


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def test_table_and_scratch_lengths():
    L = _lib.lib()
    assert L.chipq_stream_table_len(0) == 8192 and L.chipq_stream_table_len(1 << 32) == 0
    for ns in (1, 3, 6, 7, 1024):
        n = L.chipq_stream_table_len(ns)
        assert n % 16 == 0 and n >= 40 * ns + 8192 and L.chipq_stream_table_len(ns + 7) > n
    info = _lib.TableInfo(1024, 2048, 262144, 0)
    ref = ctypes.byref(info)
    for nreq, max_len in ((1, 1), (1024, 4096), (16384, 4096), (65, 5000)):
        s = L.chipq_read_scratch_len(ref, nreq, max_len, 0)
        v = L.chipq_read_scratch_len(ref, nreq, max_len, 1)
        assert s and s % 16 == 0 and v % 16 == 0 and v > s
        assert L.chipq_read_scratch_len(ref, nreq + 64, max_len, 0) > s
    # more segment slots per request where a range can span more shards
    small = _lib.TableInfo(4, 8, 1024, 0)
    assert L.chipq_read_scratch_len(ctypes.byref(small), 1024, 4096, 0) > L.chipq_read_scratch_len(ref, 1024, 4096, 0)
    for bad in ((ref, 1 << 31, 4096), (ref, 16, 0), (ref, 16, (1 << 53) + 1), (None, 16, 4096), (ref, 1 << 30, 1 << 20)):
        assert L.chipq_read_scratch_len(*bad, 1) == 0, bad[1:]
    assert L.chipq_read_scratch_len(ref, 0, 4096, 0) % 16 == 0


def test_stream_table_argument_errors_in_their_order():
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    last = _last()
    need = L.chipq_stream_table_len(3)

    def call(in_off=RC.OFF3, in_len=RC.LEN3, enc=STR, hashes=HASH, table=TAB, table_len=need, ns=3, arrays=True,
             info=True):
        out = _lib.TableInfo(9, 9, 9, 9)
        rc = L.chipq_stream_table_dev(enc, u64(in_off), u64(in_len) if arrays else None, hashes, u32(RC.PAD3),
                                      u32(RC.CL3), ns, table, table_len, ctypes.byref(out) if info else None, None)
        return rc, (out.nstreams, out.max_chunks, out.min_shard, out.reserved)

    def rc(**kw):
        code, got = call(**kw)
        assert code == OK or got == (0, 0, 0, 0)  # nothing is reported of a table that was not made
        return code

    gap = [RC.LEN3[0], RC.LEN3[1] + 8, RC.LEN3[2]]
    assert call(info=False)[0] == INVALID_ARG
    assert rc(arrays=False) == INVALID_ARG and rc(enc=None) == INVALID_ARG and rc(table=None) == INVALID_ARG
    assert rc(table=TAB + 8) == INVALID_ARG and rc(ns=1 << 32) == INVALID_ARG
    assert rc(in_off=[60, RC.OFF3[1], RC.OFF3[2]]) == INVALID_ARG
    assert rc(table_len=need - 1) == INVALID_ARG
    assert rc(in_len=gap) == TRUNCATED and rc(in_len=gap, table_len=need - 1) == INVALID_ARG
    assert rc(in_len=gap, in_off=[60, RC.OFF3[1], RC.OFF3[2]]) == INVALID_ARG
    assert rc(hashes=None) == HASH_DECODE and rc(hashes=None, in_len=gap) == TRUNCATED
    if last:
        assert rc() == last


def test_read_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    info = _lib.TableInfo(3, 72, 1024, 0)
    need = {v: L.chipq_read_scratch_len(ctypes.byref(info), 6, 4096, v) for v in (0, 1)}

    def call(vouched, table=TAB, info=info, rs=REQ, start=START, length=LEN, nreq=6, max_len=4096, out=OUT, stride=4096,
             clen=CLEN, stat=STAT, used=USED, vouch=VOUCH, flags=0, scratch=SCR, scratch_len=None):
        scratch_len = need[vouched] if scratch_len is None else scratch_len
        ref = ctypes.byref(info) if info else None
        if vouched:
            return L.chipq_read_ranges_vouched_dev(table, ref, rs, start, length, nreq, max_len, out, stride, clen, stat,
                                                   used, vouch, flags, scratch, scratch_len, None)
        assert flags == 0
        return L.chipq_read_ranges_dev(table, ref, rs, start, length, nreq, max_len, out, stride, clen, stat, used,
                                       scratch, scratch_len, None)

    for v in (0, 1):
        rc = lambda **kw: call(v, **kw)  # noqa: E731
        assert rc(nreq=0) == OK
        assert rc(nreq=0, table=None, info=None, rs=None, start=None, length=None, out=None, clen=None, stat=None,
                  used=None, vouch=None, scratch=None, max_len=0, stride=7, scratch_len=0) == OK
        for name in ("table", "info", "rs", "start", "length", "out", "clen", "stat", "used", "scratch"):
            assert rc(**{name: None}) == INVALID_ARG, name
        assert rc(nreq=1 << 31, scratch_len=1 << 60) == INVALID_ARG
        assert rc(max_len=0) == INVALID_ARG and rc(max_len=(1 << 53) + 1, stride=1 << 54, scratch_len=1 << 60) == INVALID_ARG
        assert rc(stride=4088) == INVALID_ARG and rc(stride=4080) == INVALID_ARG and rc(max_len=4097) == INVALID_ARG
        assert rc(stride=1 << 62) == INVALID_ARG                    # a slot address would wrap
        assert rc(out=OUT + 8) == INVALID_ARG and rc(scratch=SCR + 8) == INVALID_ARG and rc(table=TAB + 8) == INVALID_ARG
        assert rc(nreq=1 << 30, max_len=1 << 20, stride=1 << 20, scratch_len=1 << 60) == INVALID_ARG  # 2^36 work items
        assert rc(scratch_len=need[v] - 1) == INVALID_ARG
        if last:
            assert rc() == last and rc(stride=8192) == last
    assert need[1] > need[0]
    assert call(1, vouch=None) == INVALID_ARG
    for f in (2, 4, 3, 1 << 31):
        assert call(1, flags=f) == INVALID_ARG
    # the order: a bad stride is reported before bad flags, flags before the bounds, the bounds before the scratch
    assert call(1, flags=2, scratch_len=0) == INVALID_ARG and call(1, stride=8, flags=2) == INVALID_ARG
    if last:
        assert call(1, flags=1) == last


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "qread_plan_check.cpp", include=[CSRC])


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_qread_plan_under_asan_ubsan(plan_check, seed):
    """The request kernel's planning text on the host against read::plan_read
    record for record, the serial scan against audit::finish, every grid bound
    against the true totals (exhaustively for N <= 256, w <= 8), the segment
    slots and the order of the host checks."""
    out = B.run_check(plan_check, seed, timeout=300)
    assert out.strip().splitlines()[-1] == "0 failures"


def test_qread_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "qread_bench.py"), "--dry"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "qread_bench" and res["dry_run"] is True
    assert res["streams"] == 1024 and res["object_bytes"] == (1 << 20) - 41 and res["range_bytes"] == 4096
    assert res["read_1"]["requests"] == 1024 and res["read_16"]["requests"] == 16384
    assert res["read_1"]["segment_slots"] == 2048 and res["read_16"]["scan_workgroups_per_array"] == 33
    assert res["read_16"]["vouched_scratch_bytes"] > res["read_16"]["scratch_bytes"] > 0
    assert res["launches"] == {"plan": 4, "read": 6, "vouched_read": 8}
    assert res["uploads_per_read"] == 0 and res["memsets_per_read"] == 0
    assert res["table_bytes"] == _lib.lib().chipq_stream_table_len(1024)
