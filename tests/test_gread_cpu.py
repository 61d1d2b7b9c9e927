"""CPU tests of the gread boundary (include/carbonado_hip_gread.h): the chipg_*
symbols beside the twelve older sets, their ctypes and Rust bindings, the
errors the calls decide before they touch a device, in the header's order, the
table and scratch lengths, the bench tool's dry run, and the decision text the
kernels compile (carbonado_amd/csrc/gread_device.hpp) with the host's O(1)
share (gread_plan.hpp) as a stand-alone program under ASan + UBSan."""
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
HEADER = ROOT / "include" / "carbonado_hip_gread.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_gread.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"
CSRC = ROOT / "carbonado_amd" / "csrc"

OK, INVALID_ARG, NO_DEVICE = 0, 1, 100
NAMES = {"chipg_abi_version", "chipg_frame_table_len", "chipg_frame_table_dev", "chipg_read_scratch_len",
         "chipg_read_ranges_dev"}
# the thirteenth boundary; boundary.BOUNDARIES holds the first nine, then fread, qread and kread
MINE = B._boundary("chipg_", "gread", _lib.GREAD_SIGNATURES, 5)
OLDER = B.BOUNDARIES + (B._boundary("chipf_", "fread", _lib.FREAD_SIGNATURES, 7),
                        B._boundary("chipq_", "qread", _lib.QREAD_SIGNATURES, 6),
                        B._boundary("chipk_", "kread", _lib.KREAD_SIGNATURES, 6))
FRAME = 65536


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipg_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == MINE.exports
    exported = B.exported()
    assert set(protos) == B.exports_of(exported, MINE.prefix) == set(MINE.signatures)
    assert set(B.ffi_declarations(FFI, "chipg_")) == NAMES
    for name, (_, ps) in protos.items():
        assert len(MINE.signatures[name][1]) == len(ps), name
    assert _lib.lib().chipg_abi_version() == 1
    text = HEADER.read_text()
    assert "#define CHIPG_ABI_VERSION 1" in text
    assert '#include "carbonado_hip_kread.h"' in text and '#include "carbonado_hip_fread.h"' in text
    # every older boundary keeps its count; no prefix clashes, no shared name
    assert [b.exports for b in OLDER] == [62, 5, 6, 4, 4, 3, 10, 10, 8, 7, 6, 6]
    for b in OLDER:
        assert len(B.exports_of(exported, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(MINE.prefix) and not MINE.prefix.startswith(b.prefix)
        assert not set(MINE.signatures) & set(b.signatures), b.prefix
    # the argument lists the header states
    assert [n for n, _ in protos["chipg_frame_table_len"][1]] == ["nstreams", "nentries"]
    assert [n for n, _ in protos["chipg_frame_table_dev"][1]] == [
        "format", "chunk_len", "padding", "index_status", "frame_off", "idx_off", "nframes", "plain_len", "nstreams",
        "d_ftable", "ftable_len", "finfo", "stream"]
    assert [n for n, _ in protos["chipg_read_scratch_len"][1]] == ["info", "finfo", "nreq", "max_len"]
    assert [n for n, _ in protos["chipg_read_ranges_dev"][1]] == [
        "d_table", "info", "d_ftable", "finfo", "d_keytab", "keytab_len", "d_req_stream", "d_start", "d_len", "nreq",
        "max_len", "d_content", "content_stride", "d_content_len", "d_status", "d_used", "d_vouch", "flags", "d_scratch",
        "scratch_len", "stream"]
    # the read is kread's planned read with the frame table behind info
    k = [n for n, _ in B.prototypes(ROOT / "include" / "carbonado_hip_kread.h", "chipk_")["chipk_read_ranges_dev"][1]]
    g = [n for n, _ in protos["chipg_read_ranges_dev"][1]]
    assert g[:2] + g[4:] == k
    # the frame table takes the index arguments of the host-planned read, in its order
    f = [n for n, _ in B.prototypes(ROOT / "include" / "carbonado_hip_fread.h", "chipf_")["chipf_read_layout"][1]]
    assert [n for n, _ in protos["chipg_frame_table_dev"][1]][:9] == f[:9]
    assert ctypes.sizeof(_lib.FrameInfo) == 32 and [n for n, _ in _lib.FrameInfo._fields_] == [
        "nstreams", "nentries", "max_frame", "format"]
    assert re.search(r"typedef struct chipg_frame_info \{[^}]*uint64_t nstreams;[^}]*uint64_t nentries;[^}]*"
                     r"uint64_t max_frame;[^}]*uint64_t format;[^}]*\} chipg_frame_info;", text)


def test_ffi_gread_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipg_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPG_ABI_VERSION: c_int = 1;", text)
    assert "chipq_table_info" in text
    m = re.search(r"#\[repr\(C\)\][^{]*pub struct chipg_frame_info \{([^}]*)\}", text)
    assert m and re.findall(r"pub (\w+): u64", m.group(1)) == ["nstreams", "nentries", "max_frame", "format"]


WRAPPERS = (("frame_table_len", "frame_table", ("chipg_frame_table_len",)),
            ("frame_table", "frame_table", ("chipg_frame_table_dev",)),
            ("planned_frame_read_scratch_len", "planned_frame_read_scratch", ("chipg_read_scratch_len",)),
            ("read_frame_ranges_planned", "read_frame_ranges_planned", ("chipg_read_ranges_dev",)))


def test_lib_rs_and_device_module_have_the_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^mod ffi_gread;", lib, flags=re.M) and "chipg_abi_version" in lib
    assert re.search(r"^class FrameTable\b", src, flags=re.M)
    for rust_fn, py_fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {rust_fn}\(", lib)
        assert m, rust_fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert re.search(rf"^def {py_fn}\(", src, flags=re.M), py_fn
        for call in calls:
            assert f"ffi_gread::{call}(" in body, (rust_fn, call)
            assert f"{call}(" in src, call


# never dereferenced: the checks come first
OUT, STAT, USED, SCR = RC.OUT, RC.STAT, RC.USED, RC.SCR
TAB, REQ, START, LEN, CLEN, VOUCH, KEYS, FTAB = (0x79000000, 0x7A000000, 0x7A100000, 0x7A200000, 0x7A300000, 0x77000000,
                                                 0x7B000000, 0x7C000000)


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def _up16(x):
    return (x + 15) // 16 * 16


def test_table_and_scratch_lengths():
    L = _lib.lib()
    assert L.chipg_frame_table_len(0, 0) == 0
    assert L.chipg_frame_table_len(1 << 31, 1) == 0 and L.chipg_frame_table_len(1, 1 << 30) == 0
    assert L.chipg_frame_table_len((1 << 31) - 1, (1 << 30) - 1) > 0
    for ns, ne in ((1, 1), (2, 7), (3, 8), (5, 9), (1024, 17408)):
        n = L.chipg_frame_table_len(ns, ne)
        # one 32-B record per stream and 8 B per entry
        assert n % 16 == 0 and n == 32 * ns + _up16(8 * ne)
        assert L.chipg_frame_table_len(ns + 1, ne) > n and L.chipg_frame_table_len(ns, ne + 2) > n
    info = _lib.TableInfo(1024, 2048, 262144, 0)
    ref = ctypes.byref(info)
    for fmt in (14, 15):
        finfo = _lib.FrameInfo(1024, 17408, FRAME + 8, fmt)
        fref = ctypes.byref(finfo)
        for nreq, max_len, fcap in ((1, 1, 1), (1024, 4096, 2), (16384, 4096, 2), (65, 65537, 2), (65, 65538, 3),
                                    (65, 70000, 3)):
            s = L.chipg_read_scratch_len(ref, fref, nreq, max_len)
            inner_len = fcap * (FRAME + 8)
            inner = (L.chipk_read_scratch_len(ref, nreq, inner_len) if fmt == 15 else
                     L.chipq_read_scratch_len(ref, nreq, inner_len, 1))
            # the inner call's scratch, three request arrays, its content lengths, the verdict words, the staging slots
            body = inner + (4 + 8 + 8 + 8) * nreq + 4 * nreq * fcap + nreq * _up16(inner_len)
            assert inner and s % 16 == 0 and body <= s < body + 6 * 256, (fmt, nreq, max_len)
            assert L.chipg_read_scratch_len(ref, fref, nreq + 64, max_len) > s
            assert L.chipg_read_scratch_len(ref, fref, nreq, max_len + FRAME) > s
        for bad in ((ref, fref, 1 << 31, 4096), (ref, fref, 16, 0), (ref, fref, 16, (1 << 53) + 1), (None, fref, 16, 4096),
                    (ref, None, 16, 4096), (ref, fref, 1 << 30, 1 << 20)):
            assert L.chipg_read_scratch_len(*bad) == 0, bad[2:]
        # 2^31 block workgroups or more
        assert L.chipg_read_scratch_len(ref, fref, 1 << 20, 1 << 27) == 0
        # tables of different stream counts, a format that is none
        assert L.chipg_read_scratch_len(ref, ctypes.byref(_lib.FrameInfo(1023, 17408, FRAME + 8, fmt)), 16, 4096) == 0
        assert L.chipg_read_scratch_len(ref, ctypes.byref(_lib.FrameInfo(1024, 17408, FRAME + 8, 13)), 16, 4096) == 0
        # a table without a frame: the inner capacity is one byte
        assert L.chipg_read_scratch_len(ref, ctypes.byref(_lib.FrameInfo(1024, 1024, 0, fmt)), 16, 4096) > 0
        assert L.chipg_read_scratch_len(ref, fref, 0, 4096) % 16 == 0


def _index(ns=3):
    """Three streams of 0, 1 and 2 frames at format 14, as the calls take them."""
    cl = (ctypes.c_uint32 * 3)(1024, 1024, 65536)
    lens = [0, 10 + 20, 10 + (FRAME + 8) + 30]
    pad = (ctypes.c_uint32 * 3)(*[4 * c - n for c, n in zip(cl, lens)])
    fo = (ctypes.c_uint64 * 8)(0, 0x77, 10, 30, 0x77, 10, 10 + FRAME + 8, lens[2])
    io = (ctypes.c_uint64 * 3)(0, 2, 5)
    nf = (ctypes.c_uint64 * 3)(0, 1, 2)
    pl = (ctypes.c_uint64 * 3)(0, 7, FRAME + 3)
    return cl, pad, fo, io, nf, pl


def test_frame_table_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    cl, pad, fo, io, nf, pl = _index()
    need = L.chipg_frame_table_len(3, 6)
    assert need == 96 + 48

    def rc(fmt=14, cl=cl, pad=pad, ist=None, fo=fo, io=io, nf=nf, pl=pl, ns=3, table=FTAB, table_len=need, finfo=True):
        info = _lib.FrameInfo(9, 9, 9, 9)
        code = L.chipg_frame_table_dev(fmt, cl, pad, ist, fo, io, nf, pl, ns, table, table_len,
                                       ctypes.byref(info) if finfo else None, None)
        return code, (info.nstreams, info.nentries, info.max_frame, info.format)

    zero = (0, 0, 0, 0)
    assert rc(finfo=False)[0] == INVALID_ARG
    assert rc(fmt=13) == (INVALID_ARG, zero) and rc(fmt=13, ns=0) == (INVALID_ARG, zero)
    assert rc(ns=0) == (OK, (0, 0, 0, 14)) and rc(fmt=15, ns=0, cl=None, fo=None, table=None, table_len=0) == (OK, (0, 0, 0, 15))
    for name in ("cl", "pad", "fo", "io", "nf", "pl", "table"):
        assert rc(**{name: None}) == (INVALID_ARG, zero), name
    assert rc(ns=1 << 31) == (INVALID_ARG, zero)
    # the per-stream checks of the host-planned read: idx_off, nframes, the index
    assert rc(io=(ctypes.c_uint64 * 3)(0, (1 << 53) + 1, 5)) == (INVALID_ARG, zero)
    assert rc(nf=(ctypes.c_uint64 * 3)(0, 1 << 31, 2)) == (INVALID_ARG, zero)
    for at, v in ((6, 10), (7, 99), (3, 31), (0, 1)):           # entries that do not ascend; a last entry that is not L
        bad = (ctypes.c_uint64 * 8)(*fo)
        bad[at] = v
        assert rc(fo=bad) == (INVALID_ARG, zero), at
    for s, v in ((1, 0), (1, FRAME + 1), (2, FRAME), (2, 2 * FRAME + 1), (0, 1)):   # a plain_len that does not fit nframes
        bad = (ctypes.c_uint64 * 3)(*pl)
        bad[s] = v
        assert rc(pl=bad) == (INVALID_ARG, zero), (s, v)
    # a stream whose index_status is not 0 is not looked at, and has no entries
    bad = (ctypes.c_uint64 * 8)(*fo)
    bad[6] = 10
    ist = (ctypes.c_uint32 * 3)(0, 0, 16)
    assert rc(fo=bad, ist=ist, table_len=0)[0] == INVALID_ARG
    assert rc(table=FTAB + 8) == (INVALID_ARG, zero) and rc(table_len=need - 1) == (INVALID_ARG, zero)
    if last:
        assert rc() == (last, zero) and rc(fo=bad, ist=ist, table_len=96 + 32) == (last, zero)


def test_read_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    info = _lib.TableInfo(3, 72, 1024, 0)
    tlen = L.chipk_key_table_len(3)
    for fmt in (14, 15):
        finfo = _lib.FrameInfo(3, 6, FRAME + 8, fmt)
        need = L.chipg_read_scratch_len(ctypes.byref(info), ctypes.byref(finfo), 6, 4096)
        assert need > 6 * 2 * (FRAME + 8)

        def rc(table=TAB, info=info, ftab=FTAB, finfo=finfo, keytab=KEYS, keytab_len=tlen, rs=REQ, start=START, length=LEN,
               nreq=6, max_len=4096, out=OUT, stride=4096, clen=CLEN, stat=STAT, used=USED, vouch=VOUCH, flags=0,
               scratch=SCR, scratch_len=need):
            ref = ctypes.byref(info) if info else None
            fref = ctypes.byref(finfo) if finfo else None
            return L.chipg_read_ranges_dev(table, ref, ftab, fref, keytab, keytab_len, rs, start, length, nreq, max_len, out,
                                           stride, clen, stat, used, vouch, flags, scratch, scratch_len, None)

        assert rc(nreq=0) == OK
        assert rc(nreq=0, table=None, info=None, ftab=None, finfo=None, keytab=None, keytab_len=0, rs=None, start=None,
                  length=None, out=None, clen=None, stat=None, used=None, vouch=None, scratch=None, max_len=0, stride=7,
                  scratch_len=0) == OK
        for name in ("table", "info", "ftab", "finfo", "rs", "start", "length", "out", "clen", "stat", "used", "vouch",
                     "scratch"):
            assert rc(**{name: None}) == INVALID_ARG, name
        for f in (0, 12, 13, 16, 14 + (1 << 32)):
            assert rc(finfo=_lib.FrameInfo(3, 6, FRAME + 8, f)) == INVALID_ARG, f
        # d_keytab and keytab_len count at 15 only
        for kw in (dict(keytab=None), dict(keytab=KEYS + 8), dict(keytab_len=tlen - 1), dict(keytab_len=0)):
            if fmt == 15:
                assert rc(**kw) == INVALID_ARG, kw
            elif last:
                assert rc(**kw) == last, kw
        assert rc(nreq=1 << 31, scratch_len=1 << 60) == INVALID_ARG
        assert rc(max_len=0) == INVALID_ARG and rc(max_len=(1 << 53) + 1, stride=1 << 54, scratch_len=1 << 60) == INVALID_ARG
        assert rc(stride=4088) == INVALID_ARG and rc(stride=4080) == INVALID_ARG and rc(max_len=4097) == INVALID_ARG
        assert rc(stride=1 << 62) == INVALID_ARG                    # a slot address would wrap
        assert rc(out=OUT + 8) == INVALID_ARG and rc(scratch=SCR + 8) == INVALID_ARG and rc(table=TAB + 8) == INVALID_ARG
        for f in (2, 4, 3, 1 << 31):
            assert rc(flags=f) == INVALID_ARG
        assert rc(nreq=1 << 30, max_len=1 << 20, stride=1 << 20, scratch_len=1 << 60) == INVALID_ARG  # 2^36 work items
        # the inner capacity: above 2^53; bounds that the outer capacity passes
        assert rc(finfo=_lib.FrameInfo(3, 6, 1 << 53, fmt), scratch_len=1 << 60) == INVALID_ARG
        assert rc(finfo=_lib.FrameInfo(3, 6, 1 << 40, fmt), scratch_len=1 << 62) == INVALID_ARG
        assert rc(ftab=FTAB + 8) == INVALID_ARG
        assert rc(finfo=_lib.FrameInfo(4, 6, FRAME + 8, fmt), scratch_len=1 << 60) == INVALID_ARG
        assert rc(info=_lib.TableInfo(2, 72, 1024, 0), scratch_len=1 << 60) == INVALID_ARG
        assert rc(nreq=1 << 20, max_len=1 << 27, stride=1 << 27, scratch_len=1 << 62) == INVALID_ARG  # 2^31 workgroups
        assert rc(scratch_len=need - 1) == INVALID_ARG and rc(scratch_len=0) == INVALID_ARG
        # every one of them before the device
        assert rc(flags=2, scratch_len=0) == INVALID_ARG and rc(stride=8, flags=2) == INVALID_ARG
        if last:
            assert rc() == last and rc(stride=8192) == last and rc(flags=1) == last
            assert rc(keytab_len=tlen + 16) == last
            assert rc(finfo=_lib.FrameInfo(3, 3, 0, fmt)) == last   # no frame at all: served


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "gread_plan_check.cpp", include=[CSRC])


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_gread_plan_under_asan_ubsan(plan_check, seed):
    """The rewrite's decision text on the host against fread::plan_ranges
    request by request, the register-built work item of every (r, k) against
    fread::plan_items' Seg field for field, fcap against a brute-force count of
    touched frames, the frame table's checks, max_frame and layout, the
    scratch's layout and the order of the host checks."""
    out = B.run_check(plan_check, seed, timeout=300)
    assert out.strip().splitlines()[-1] == "0 failures"


def test_gread_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gread_bench.py"), "--dry"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    L = _lib.lib()
    assert res["tool"] == "gread_bench" and res["dry_run"] is True
    assert res["streams"] == 1024 and res["object_bytes"] == 1 << 20 and res["range_bytes"] == 4096
    assert res["frames_per_stream"] == 16 and res["max_frame"] == FRAME + 8 and res["fcap"] == 2
    assert res["launches"]["14"]["total"] == 15 == sum(v for k, v in res["launches"]["14"].items() if k != "total")
    assert res["launches"]["15"]["total"] == 17 == sum(v for k, v in res["launches"]["15"].items() if k != "total")
    assert res["uploads_per_read"] == 0 and res["memsets_per_read"] == 0
    assert res["frame_table_bytes"] == L.chipg_frame_table_len(1024, 1024 * 17) == 32 * 1024 + 8 * 17 * 1024
    assert res["key_table_bytes"] == L.chipk_key_table_len(1024)
    assert res["stream_table_bytes"] == L.chipq_stream_table_len(1024)
    for fmt in (14, 15):
        lv = res[f"level{fmt}"]
        info = _lib.TableInfo(1024, lv["max_chunks"], lv["min_shard"], 0)
        finfo = _lib.FrameInfo(1024, 1024 * 17, FRAME + 8, fmt)
        assert lv["min_shard"] % 1024 == 0 and lv["max_chunks"] == 8 * lv["min_shard"] // 1024
        for key, nreq in (("read_1", 1024), ("read_16", 16384)):
            assert lv[key]["requests"] == nreq and lv[key]["block_workgroups"] == 2 * nreq
            assert lv[key]["scratch_bytes"] == L.chipg_read_scratch_len(ctypes.byref(info), ctypes.byref(finfo), nreq, 4096)
            assert lv[key]["staging_bytes"] == nreq * _up16(2 * (FRAME + 8)) < lv[key]["scratch_bytes"]
            assert lv[key]["damaged_streams"] == 16
