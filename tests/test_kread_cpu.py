"""CPU tests of the kread boundary (include/carbonado_hip_kread.h): the chipk_*
symbols beside the eleven older sets, their ctypes and Rust bindings, the
errors the calls decide before they touch a device, in the header's order, the
table and scratch lengths, the bench tool's dry run, and the decision text the
kernels compile (carbonado_amd/csrc/kread_device.hpp) with the host's O(1)
share (kread_plan.hpp) as a stand-alone program under ASan + UBSan."""
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
HEADER = ROOT / "include" / "carbonado_hip_kread.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_kread.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"
CSRC = ROOT / "carbonado_amd" / "csrc"

OK, INVALID_ARG, NO_DEVICE = 0, 1, 100
NAMES = {"chipk_abi_version", "chipk_key_table_len", "chipk_key_table_dev", "chipk_key_table_wipe_dev",
         "chipk_read_scratch_len", "chipk_read_ranges_dev"}
# the twelfth boundary; boundary.BOUNDARIES holds the first nine, test_fread_cpu the tenth, test_qread_cpu the eleventh
MINE = B._boundary("chipk_", "kread", _lib.KREAD_SIGNATURES, 6)
OLDER = B.BOUNDARIES + (B._boundary("chipf_", "fread", _lib.FREAD_SIGNATURES, 7),
                        B._boundary("chipq_", "qread", _lib.QREAD_SIGNATURES, 6))


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipk_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == MINE.exports
    exported = B.exported()
    assert set(protos) == B.exports_of(exported, MINE.prefix) == set(MINE.signatures)
    assert set(B.ffi_declarations(FFI, "chipk_")) == NAMES
    for name, (_, ps) in protos.items():
        assert len(MINE.signatures[name][1]) == len(ps), name
    assert _lib.lib().chipk_abi_version() == 1
    text = HEADER.read_text()
    assert "#define CHIPK_ABI_VERSION 1" in text
    assert '#include "carbonado_hip_qread.h"' in text and '#include "carbonado_hip_cread.h"' in text
    # every older boundary keeps its count; no prefix clashes, no shared name
    assert [b.exports for b in OLDER] == [62, 5, 6, 4, 4, 3, 10, 10, 8, 7, 6]
    for b in OLDER:
        assert len(B.exports_of(exported, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(MINE.prefix) and not MINE.prefix.startswith(b.prefix)
        assert not set(MINE.signatures) & set(b.signatures), b.prefix
    # the argument lists the header states
    assert [n for n, _ in protos["chipk_key_table_len"][1]] == ["nstreams"]
    assert [n for n, _ in protos["chipk_key_table_dev"][1]] == ["keys", "ivs", "key_status", "nstreams", "d_keytab",
                                                                "keytab_len", "stream"]
    assert [n for n, _ in protos["chipk_key_table_wipe_dev"][1]] == ["d_keytab", "keytab_len", "stream"]
    assert [n for n, _ in protos["chipk_read_scratch_len"][1]] == ["info", "nreq", "max_len"]
    assert [n for n, _ in protos["chipk_read_ranges_dev"][1]] == [
        "d_table", "info", "d_keytab", "keytab_len", "d_req_stream", "d_start", "d_len", "nreq", "max_len", "d_content",
        "content_stride", "d_content_len", "d_status", "d_used", "d_vouch", "flags", "d_scratch", "scratch_len", "stream"]
    # the read is the vouched planned read with the key table behind info
    q = [n for n, _ in B.prototypes(ROOT / "include" / "carbonado_hip_qread.h", "chipq_")["chipq_read_ranges_vouched_dev"][1]]
    k = [n for n, _ in protos["chipk_read_ranges_dev"][1]]
    assert k[:2] + k[4:] == q


def test_ffi_kread_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipk_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPK_ABI_VERSION: c_int = 1;", text)
    assert "chipq_table_info" in text and "struct" not in text  # the one struct is qread's


WRAPPERS = (("key_table_len", "key_table", ("chipk_key_table_len",)),
            ("key_table", "key_table", ("chipk_key_table_dev",)),
            ("wipe_key_table", "wipe_key_table", ("chipk_key_table_wipe_dev",)),
            ("planned_plain_read_scratch_len", "planned_plain_read_scratch", ("chipk_read_scratch_len",)),
            ("read_plain_ranges_planned", "read_plain_ranges_planned", ("chipk_read_ranges_dev",)))


def test_lib_rs_and_device_module_have_the_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^mod ffi_kread;", lib, flags=re.M) and "chipk_abi_version" in lib
    assert re.search(r"^class KeyTable\b", src, flags=re.M)
    for rust_fn, py_fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {rust_fn}\(", lib)
        assert m, rust_fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert re.search(rf"^def {py_fn}\(", src, flags=re.M), py_fn
        for call in calls:
            assert f"ffi_kread::{call}(" in body, (rust_fn, call)
            assert f"{call}(" in src, call


# never dereferenced: the checks come first
OUT, STAT, USED, SCR = RC.OUT, RC.STAT, RC.USED, RC.SCR
TAB, REQ, START, LEN, CLEN, VOUCH, KEYS = (0x79000000, 0x7A000000, 0x7A100000, 0x7A200000, 0x7A300000, 0x77000000,
                                           0x7B000000)


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def test_table_and_scratch_lengths():
    L = _lib.lib()
    assert L.chipk_key_table_len(0) == 0 and L.chipk_key_table_len(1 << 32) == 0
    assert L.chipk_key_table_len((1 << 32) - 1) > 0
    for ns in (1, 2, 3, 5, 6, 7, 1024):
        n = L.chipk_key_table_len(ns)
        # one 512-B record, one status word and one raw key || IV record per stream
        assert n % 16 == 0 and 564 * ns <= n < 564 * ns + 16 and L.chipk_key_table_len(ns + 1) > n
    info = _lib.TableInfo(1024, 2048, 262144, 0)
    ref = ctypes.byref(info)
    for nreq, max_len in ((1, 1), (1024, 4096), (16384, 4096), (65, 5000)):
        s = L.chipk_read_scratch_len(ref, nreq, max_len)
        q = L.chipq_read_scratch_len(ref, nreq, max_len, 1)
        # qread's vouched scratch and three request arrays behind it
        assert s % 16 == 0 and s >= q + 20 * nreq and s < q + 20 * nreq + 4 * 256
        assert L.chipk_read_scratch_len(ref, nreq + 64, max_len) > s
    for bad in ((ref, 1 << 31, 4096), (ref, 16, 0), (ref, 16, (1 << 53) + 1), (None, 16, 4096), (ref, 1 << 30, 1 << 20)):
        assert L.chipk_read_scratch_len(*bad) == 0, bad[1:]
    # 2^31 keystream waves or more, where qread's own bounds still hold
    big = _lib.TableInfo(3, 8, 1 << 30, 0)
    assert L.chipq_read_scratch_len(ctypes.byref(big), 1 << 20, 4 << 20, 1) > 0
    assert L.chipk_read_scratch_len(ctypes.byref(big), 1 << 20, 4 << 20) == 0
    assert L.chipk_read_scratch_len(ref, 0, 4096) % 16 == 0


def test_key_table_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    need = L.chipk_key_table_len(3)
    keys = (ctypes.c_uint8 * 96)(*range(96))
    ivs = (ctypes.c_uint8 * 48)(*range(48))
    ks = (ctypes.c_uint32 * 3)(0, 17, 0)

    def rc(keys=keys, ivs=ivs, ks=ks, ns=3, table=KEYS, table_len=need):
        return L.chipk_key_table_dev(keys, ivs, ks, ns, table, table_len, None)

    assert rc(ns=0) == OK and rc(ns=0, keys=None, ivs=None, ks=None, table=None, table_len=0) == OK
    assert rc(keys=None) == INVALID_ARG and rc(ivs=None) == INVALID_ARG and rc(table=None) == INVALID_ARG
    assert rc(table=KEYS + 8) == INVALID_ARG and rc(ns=1 << 32, table_len=1 << 60) == INVALID_ARG
    assert rc(table_len=need - 1) == INVALID_ARG and rc(table_len=0) == INVALID_ARG
    assert rc(ks=None, table_len=need - 1) == INVALID_ARG   # a NULL key_status is no error of its own
    if last:
        assert rc() == last and rc(ks=None) == last
    # the wipe
    assert L.chipk_key_table_wipe_dev(None, 0, None) == OK and L.chipk_key_table_wipe_dev(KEYS, 0, None) == OK
    assert L.chipk_key_table_wipe_dev(None, need, None) == INVALID_ARG
    if last:
        assert L.chipk_key_table_wipe_dev(KEYS, need, None) == last


def test_read_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    info = _lib.TableInfo(3, 72, 1024, 0)
    need = L.chipk_read_scratch_len(ctypes.byref(info), 6, 4096)
    tlen = L.chipk_key_table_len(3)
    assert need > L.chipq_read_scratch_len(ctypes.byref(info), 6, 4096, 1)

    def rc(table=TAB, info=info, keytab=KEYS, keytab_len=tlen, rs=REQ, start=START, length=LEN, nreq=6, max_len=4096,
           out=OUT, stride=4096, clen=CLEN, stat=STAT, used=USED, vouch=VOUCH, flags=0, scratch=SCR, scratch_len=need):
        ref = ctypes.byref(info) if info else None
        return L.chipk_read_ranges_dev(table, ref, keytab, keytab_len, rs, start, length, nreq, max_len, out, stride,
                                       clen, stat, used, vouch, flags, scratch, scratch_len, None)

    assert rc(nreq=0) == OK
    assert rc(nreq=0, table=None, info=None, keytab=None, keytab_len=0, rs=None, start=None, length=None, out=None,
              clen=None, stat=None, used=None, vouch=None, scratch=None, max_len=0, stride=7, scratch_len=0) == OK
    for name in ("table", "info", "keytab", "rs", "start", "length", "out", "clen", "stat", "used", "vouch", "scratch"):
        assert rc(**{name: None}) == INVALID_ARG, name
    assert rc(nreq=1 << 31, scratch_len=1 << 60) == INVALID_ARG
    assert rc(max_len=0) == INVALID_ARG and rc(max_len=(1 << 53) + 1, stride=1 << 54, scratch_len=1 << 60) == INVALID_ARG
    assert rc(stride=4088) == INVALID_ARG and rc(stride=4080) == INVALID_ARG and rc(max_len=4097) == INVALID_ARG
    assert rc(stride=1 << 62) == INVALID_ARG                    # a slot address would wrap
    assert rc(out=OUT + 8) == INVALID_ARG and rc(scratch=SCR + 8) == INVALID_ARG and rc(table=TAB + 8) == INVALID_ARG
    assert rc(keytab=KEYS + 8) == INVALID_ARG and rc(keytab_len=tlen - 1) == INVALID_ARG and rc(keytab_len=0) == INVALID_ARG
    for f in (2, 4, 3, 1 << 31):
        assert rc(flags=f) == INVALID_ARG
    assert rc(nreq=1 << 30, max_len=1 << 20, stride=1 << 20, scratch_len=1 << 60) == INVALID_ARG  # 2^36 work items
    big = _lib.TableInfo(3, 8, 1 << 30, 0)
    assert rc(info=big, nreq=1 << 20, max_len=4 << 20, stride=4 << 20, scratch_len=1 << 60) == INVALID_ARG  # 2^31 waves
    assert rc(scratch_len=need - 1) == INVALID_ARG
    assert rc(scratch_len=L.chipq_read_scratch_len(ctypes.byref(info), 6, 4096, 1)) == INVALID_ARG
    # every one of them before the device
    assert rc(flags=2, scratch_len=0) == INVALID_ARG and rc(stride=8, flags=2) == INVALID_ARG
    if last:
        assert rc() == last and rc(stride=8192) == last and rc(flags=1) == last
        assert rc(keytab_len=tlen + 16) == last


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "kread_plan_check.cpp", include=[CSRC])


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_kread_plan_under_asan_ubsan(plan_check, seed):
    """The rewrite's decision text on the host against cread::shifted and the
    host call's own decisions request by request, the bounded work mapping
    against the host-planned item split byte for byte, the key table's and the
    scratch's layout and the order of the host checks."""
    out = B.run_check(plan_check, seed, timeout=300)
    assert out.strip().splitlines()[-1] == "0 failures"


def test_kread_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "kread_bench.py"), "--dry"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    L = _lib.lib()
    assert res["tool"] == "kread_bench" and res["dry_run"] is True
    assert res["streams"] == 1024 and res["envelope_bytes"] == (1 << 20) - 41 and res["range_bytes"] == 4096
    assert res["read_1"]["requests"] == 1024 and res["read_16"]["requests"] == 16384
    info = _lib.TableInfo(1024, res["max_chunks"], res["min_shard"], 0)
    assert (res["max_chunks"], res["min_shard"]) == (2048, 262144)
    for key, nreq in (("read_1", 1024), ("read_16", 16384)):
        assert res[key]["scratch_bytes"] == L.chipk_read_scratch_len(ctypes.byref(info), nreq, 4096)
        assert res[key]["keystream_waves"] == 3 * nreq and res[key]["damaged_streams"] == 16
    assert res["launches"] == {"rewrite": 1, "plan": 4, "vouched_read": 8, "keystream": 1, "total": 14}
    assert res["key_table_launches"] == 2
    assert res["uploads_per_read"] == 0 and res["memsets_per_read"] == 0
    assert res["key_table_bytes"] == L.chipk_key_table_len(1024)
    assert res["stream_table_bytes"] == L.chipq_stream_table_len(1024)
